"""Identities between the LSTM kernels that hold bit for bit because every
one of them runs the same forward cell and the same backward cell
(lstm_cell_fwd / lstm_cell_bwd in ops/hip/lstm_gates.hip). An edit that
changes the cell in one kernel only breaks them. GPU-only.

- the f32 and the bf16 tail kernels differ in how a gate is loaded and how a
  gate gradient is stored, and in nothing else;
- the train forward is the no-grad forward plus its stashes: narrow against
  narrow at H = 64 and 123, wide against wide at 257 and 512, and at 128 the
  wide train forward against the narrow no-grad forward (both sum a column
  of h @ Wh sequentially over k in f32, x-projection last).

All of these pairs were bit-equal before the cell was shared as well; none
had to be left out.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H_TAIL = 5, 7  # odd H, one partial block


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available(), "HIP extension must be built on the GPU box"
    return ops.require_ext()


@pytest.fixture(scope="module")
def tail_inputs():
    torch.manual_seed(41)
    g16 = torch.randn(N, 4 * H_TAIL, device=DEV).to(torch.bfloat16)
    c = torch.randn(N, H_TAIL, device=DEV)
    gh = torch.randn(N, H_TAIL, device=DEV)
    gc = torch.randn(N, H_TAIL, device=DEV)
    return g16, c, gh, gc


def test_tail_fwd_f32_equals_bf16(ext, tail_inputs):
    g16, c, _, _ = tail_inputs
    out16 = ext.lstm_tail_fwd(g16, c, 1.0)
    out32 = ext.lstm_tail_fwd(g16.float(), c, 1.0)
    for name, a, b in zip(("new_h", "new_c", "stash"), out16, out32):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("with_grad_c", [False, True])
def test_tail_bwd_bf16_is_the_rounded_f32(ext, tail_inputs, with_grad_c):
    g16, c, gh, gc = tail_inputs
    _, new_c, stash = ext.lstm_tail_fwd(g16, c, 1.0)
    grad_c = gc if with_grad_c else None
    dg32, dc32 = ext.lstm_tail_bwd(gh, grad_c, stash, c, new_c, False)
    dg16, dc16 = ext.lstm_tail_bwd(gh, grad_c, stash, c, new_c, True)
    assert dg32.dtype == torch.float32 and dg16.dtype == torch.bfloat16
    assert torch.equal(dg16, dg32.to(torch.bfloat16))
    assert torch.equal(dc16, dc32)


@pytest.mark.parametrize("H", [64, 123, 128, 257, 512])
def test_train_fwd_equals_no_grad_fwd(ext, H):
    B, L = 2, 3
    torch.manual_seed(43 + H)
    xg = (torch.randn(B, L, 4 * H, device=DEV) * 0.5).to(torch.bfloat16)
    wh = (torch.randn(H, 4 * H, device=DEV) * (1.6 / H ** 0.5)).to(
        torch.bfloat16)
    h0 = torch.randn(B, H, device=DEV)
    c0 = torch.randn(B, H, device=DEV)
    done = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    done[0, 1] = True
    h_out, h_fin, c_fin, acts, c_prev, _ = ext.lstm_seq_train_fwd(
        xg, wh, h0, c0, done, 1.0)
    ref = ext.lstm_seq_fwd(xg, wh, h0, c0, done, 1.0)
    for name, a, b in zip(("h_out", "h_fin", "c_fin"),
                          (h_out, h_fin, c_fin), ref):
        assert torch.equal(a, b), name

    # the stash holds the cell: c' = f*c_prev + i*g is the next step's
    # c_prev (c_fin after the last step) unless a done zeroed the carry.
    # The kernel may fuse either product into the add, so it is within one
    # rounding of the product and one of the sum: 2^-23 (|f*c| + |i*g|).
    i, g, f, _ = acts.double().chunk(4, dim=2)
    fc, ig = f * c_prev.double(), i * g
    c_next = torch.cat([c_prev[:, 1:], c_fin.unsqueeze(1)], dim=1).double()
    bound = 2.0 ** -23 * (fc.abs() + ig.abs())
    keep = ~done.unsqueeze(2)
    assert bool((((fc + ig) - c_next).abs() <= bound)[keep.expand_as(fc)]
                .all())
    assert bool((c_next[done] == 0).all())
