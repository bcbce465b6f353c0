"""Double-buffered static inputs selected by a device slot word: the four
forward kernels that read static inputs (conv l1 / l1_c1, embed MLP, LSTM
tail, V-trace loss), one captured graph following the word, and the
pipelined GraphedImpalaStep against a synchronous twin. Every per-launcher
comparison is torch.equal: a slot changes an address, nothing else."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    return ops.require_ext()


def _word(v):
    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _check_launcher(call, pair_names, make_pair):
    """call(tensors: dict, slot, dist: dict) -> list of output tensors.
    pair_names: the slotted inputs; make_pair(name, seed) -> [2, ...] tensor
    with different valid data in the two sets."""
    pairs = {k: make_pair(k, 1) for k in pair_names}
    dist = {k: v[0].numel() for k, v in pairs.items()}
    none = {k: 0 for k in pair_names}
    for s in (0, 1):
        plain = call({k: v[s].clone() for k, v in pairs.items()}, None, none)
        got = call({k: v[0] for k, v in pairs.items()}, _word(s), dist)
        _same(got, plain)
        # the other set is not read: rewrite it, nothing changes
        for k, v in pairs.items():
            v[1 - s].copy_(make_pair(k, 7 + s)[1 - s])
        again = call({k: v[0] for k, v in pairs.items()}, _word(s), dist)
        _same(again, plain)
    # slot=None on set 0 is today's call
    _same(call({k: v[0] for k, v in pairs.items()}, None, none),
          call({k: v[0].clone() for k, v in pairs.items()}, None, none))


def _sd(slot, *d):
    return dict(slot=slot, slot_dist=list(d) if slot is not None else [])


# ---- conv l1, N = 3 frames: M = 1200 rows, a partial 128-row tile ---------

@pytest.mark.parametrize("layer,C", [(0, 4), (1, 1)])
def test_conv_l1_slot(ext, layer, C):
    N = 3
    torch.manual_seed(layer)
    w = (torch.randn(32, 8 * 8 * C, device="cuda") * 0.05).bfloat16()
    b = (torch.randn(32, device="cuda") * 0.1).bfloat16()

    def make(name, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randint(0, 256, (2, N, 84, 84, C), dtype=torch.uint8,
                             device="cuda", generator=g)

    def call(t, slot, d):
        y, x_st = ext.conv_fwd(layer, t["x"], w, b, True, None,
                               **_sd(slot, d["x"]))
        return [y, x_st]

    _check_launcher(call, ["x"], make)


# ---- embed MLP, N = 17 = one row tile + 1, A = 6 -------------------------

@pytest.mark.parametrize("slab_mode", [False, True])
def test_embed_slot(ext, slab_mode):
    N, A, H, EMB_COL = 17, 6, 32, 64
    torch.manual_seed(2)
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.5).bfloat16()
    table, b1, w2, b2 = mk(A, 256), mk(256), mk(256, 256), mk(256)

    def make(name, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        if name == "pa":
            return torch.randint(0, A, (2, N), device="cuda", generator=g)
        return torch.randn(2, N, H, device="cuda", generator=g)

    def call(t, slot, d):
        if slab_mode:
            slab = torch.zeros(N, EMB_COL + 256 + H + 8, device="cuda",
                               dtype=torch.bfloat16)
            res = ext.embed_mlp_fwd(t["pa"], table, b1, w2, b2,
                                    stash_idx=True, xh_slab=slab,
                                    emb_col=EMB_COL, h=t["h"],
                                    **_sd(slot, d["pa"], d["h"]))
            return [slab] + list(res[1:])
        res = ext.embed_mlp_fwd(t["pa"], table, b1, w2, b2, stash_idx=True,
                                **_sd(slot, d["pa"], 0))
        return list(res)

    _check_launcher(call, ["pa", "h"] if slab_mode else ["pa"], make)


# ---- LSTM tail, N = 17, H = 32 -------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lstm_tail_slot(ext, dtype):
    N, H = 17, 32
    torch.manual_seed(3)
    gates = torch.randn(N, 4 * H, device="cuda").to(dtype)

    def make(name, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn(2, N, H, device="cuda", generator=g)

    def call(t, slot, d):
        return list(ext.lstm_tail_fwd(gates, t["c"], 1.0, stash_c=True,
                                      **_sd(slot, d["c"])))

    _check_launcher(call, ["c"], make)


# ---- V-trace loss, B = 3, T = 3, A = 6 -----------------------------------

def _vtrace_pair(name, seed, B=3, T=3, A=6):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if name == "mu":
        return torch.softmax(
            torch.randn(2, B, T, A, device="cuda", generator=g), -1)
    if name == "act":
        return torch.randint(0, A, (2, B, T), device="cuda",
                             generator=g).int()
    if name == "rew":
        return torch.randn(2, B, T, device="cuda", generator=g)
    return torch.rand(2, B, T, device="cuda", generator=g) < 0.3


def test_vtrace_loss_slot(ext):
    B, T, A = 3, 3, 6
    torch.manual_seed(4)
    logits = torch.randn(B, T, A, device="cuda")
    value = torch.randn(B, T, device="cuda")

    def call(t, slot, d):
        return list(ext.vtrace_loss_fwd(
            logits, value, t["mu"], t["act"], t["rew"], t["done"], 0.99, 0,
            1.0, 0.05, nofill=True, stash_actions=True,
            **_sd(slot, d["mu"], d["act"], d["rew"], d["done"])))

    _check_launcher(call, ["mu", "act", "rew", "done"], _vtrace_pair)


# ---- one captured graph, the word set to 0, 1, 0 --------------------------

def test_one_graph_follows_the_word(ext):
    torch.manual_seed(5)
    N, A, H = 17, 6, 32
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.5).bfloat16()
    w1 = (torch.randn(32, 256, device="cuda") * 0.05).bfloat16()
    bc = (torch.randn(32, device="cuda") * 0.1).bfloat16()
    table, b1, w2, b2 = mk(A, 256), mk(256), mk(256, 256), mk(256)
    gates = torch.randn(N, 4 * H, device="cuda").bfloat16()
    logits = torch.randn(3, 3, A, device="cuda")
    value = torch.randn(3, 3, device="cuda")
    x = torch.randint(0, 256, (2, 3, 84, 84, 4), dtype=torch.uint8,
                      device="cuda")
    pa = torch.randint(0, A, (2, N), device="cuda")
    c = torch.randn(2, N, H, device="cuda")
    vt = {k: _vtrace_pair(k, 11) for k in ("mu", "act", "rew", "done")}
    word = _word(0)

    def launches(slot, s):
        d = (lambda t: t[0].numel()) if slot is not None else (lambda t: 0)
        out = list(ext.conv_fwd(0, x[s], w1, bc, True, None,
                                **_sd(slot, d(x))))
        out += list(ext.embed_mlp_fwd(pa[s], table, b1, w2, b2,
                                      stash_idx=True, **_sd(slot, d(pa), 0)))
        out += list(ext.lstm_tail_fwd(gates, c[s], 1.0, stash_c=True,
                                      **_sd(slot, d(c))))
        out += list(ext.vtrace_loss_fwd(
            logits, value, vt["mu"][s], vt["act"][s], vt["rew"][s],
            vt["done"][s], 0.99, 0, 1.0, 0.05, nofill=True,
            stash_actions=True,
            **_sd(slot, d(vt["mu"]), d(vt["act"]), d(vt["rew"]),
                  d(vt["done"]))))
        return out

    ref = [[t.clone() for t in launches(None, s)] for s in (0, 1)]
    assert not torch.equal(ref[0][0], ref[1][0])
    launches(word, 0)  # warm (persistent buffers) before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = launches(word, 0)
    for s in (0, 1, 0):
        word.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        _same(outs, ref[s])


# ---- GraphedImpalaStep ----------------------------------------------------

def _agent(A, H, T):
    from distributed_reinforcement_learning_amd.agents import impala
    return impala.Agent(
        trajectory=T, input_shape=[84, 84, 4], num_action=A,
        lstm_hidden_size=H, discount_factor=0.99, start_learning_rate=1e-3,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", device="cuda:0", seed=0)


def _batch(B, T, A, H, seed):
    rng = np.random.default_rng(seed)
    return dict(
        state=rng.integers(0, 255, (B, T, 84, 84, 4), dtype=np.uint8),
        reward=rng.normal(size=(B, T)).astype(np.float32),
        action=rng.integers(0, A, (B, T)).astype(np.int32),
        done=rng.random((B, T)) < 0.1,
        behavior_policy=np.full((B, T, A), 1 / A, dtype=np.float32),
        previous_action=rng.integers(0, A, (B, T)).astype(np.int64),
        initial_h=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
        initial_c=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
    )


def _twins(A, H, B, T):
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedImpalaStep,
    )
    a_pipe, a_sync = _agent(A, H, T), _agent(A, H, T)
    a_sync.model.load_state_dict(a_pipe.model.state_dict())
    a_sync.optimizer.flat_params.copy_(a_pipe.optimizer.flat_params)
    g_pipe = GraphedImpalaStep(a_pipe, batch_size=B)
    g_sync = GraphedImpalaStep(a_sync, batch_size=B)
    assert g_pipe._double, "the fused model must take the two-set path"
    return a_pipe, a_sync, g_pipe, g_sync


def _compare(g_pipe, g_sync, call, consumed):
    call()
    out_p = g_pipe.last_losses()
    g_sync.step(batch=consumed)
    out_s = g_sync.last_losses()
    # the tolerances of test_pipelined_steps_match_synchronous_steps
    for i in range(3):
        assert out_p[i] == pytest.approx(out_s[i], rel=5e-2, abs=5e-1)
    assert out_p[3] == out_s[3]
    # the set the host believes current is the one the replay read
    assert int(g_pipe._slot_word.item()) in (0, 1)


def _finish(a_pipe, a_sync, g_pipe):
    g_pipe.wait_pinned_free()
    torch.cuda.synchronize()
    assert torch.allclose(a_pipe.optimizer.flat_params,
                          a_sync.optimizer.flat_params, atol=1e-2)


def test_pipelined_five_batches_match_synchronous_twin():
    """X, Y, Z, W, V through step(pinned_src=...) are consumed as X, X, Y,
    Z, W: each set is written at least twice."""
    A, H, B, T = 6, 32, 4, 8
    a_pipe, a_sync, g_pipe, g_sync = _twins(A, H, B, T)
    batches = [_batch(B, T, A, H, seed=s) for s in range(5)]
    staged = [{k: torch.as_tensor(np.asarray(b[k])).to(v.dtype).pin_memory()
               for k, v in g_pipe.pinned.items()} for b in batches]
    consumed = [batches[0]] + batches[:4]
    read = []
    for src, c in zip(staged, consumed):
        _compare(g_pipe, g_sync, lambda: g_pipe.step(pinned_src=src), c)
        read.append(int(g_pipe._slot_word.item()))
    assert read == [0, 0, 1, 0, 1]
    _finish(a_pipe, a_sync, g_pipe)


def test_batch_call_in_the_middle_keeps_host_and_device_in_step():
    """pinned X, Y; batch= Q; pinned Z, W: consumed X, X, Q, Q, Z. After
    every call the set the host holds current is where the next replay's
    data lies, and the word the replay read names the set that held what it
    consumed."""
    A, H, B, T = 6, 32, 4, 8
    a_pipe, a_sync, g_pipe, g_sync = _twins(A, H, B, T)
    X, Y, Q, Z, W = (_batch(B, T, A, H, seed=10 + s) for s in range(5))

    def pin(b):
        return {k: torch.as_tensor(np.asarray(b[k])).to(v.dtype).pin_memory()
                for k, v in g_pipe.pinned.items()}

    sx, sy, sz, sw = pin(X), pin(Y), pin(Z), pin(W)
    plan = [(lambda: g_pipe.step(pinned_src=sx), X),
            (lambda: g_pipe.step(pinned_src=sy), X),
            (lambda: g_pipe.step(batch=Q), Q),
            (lambda: g_pipe.step(pinned_src=sz), Q),
            (lambda: g_pipe.step(pinned_src=sw), Z)]
    for call, consumed in plan:
        _compare(g_pipe, g_sync, call, consumed)
        read = int(g_pipe._slot_word.item())
        torch.cuda.synchronize()
        # the set the replay read held exactly what it was meant to consume
        # unless this call's own upload has since gone into the OTHER set
        dev = g_pipe._sets[read]["action"].cpu().numpy()
        assert np.array_equal(dev, consumed["action"])
    _finish(a_pipe, a_sync, g_pipe)
