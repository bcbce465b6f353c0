"""The torch reference of the LSTM sequence kernels, shared by the GPU tests
that check them (models/blocks.LSTMCellTF semantics: gate order [i, g, f, o],
forget bias on f, done mask on the carry and not on the emitted h)."""

import torch


def lstm_seq_reference(xg, wh, h0, c0, done):
    """fp32 torch loop on the same bf16 inputs; forget bias 1.0."""
    h, c = h0, c0
    outs = []
    for t in range(xg.shape[1]):
        gates = xg[:, t].float() + h.float() @ wh.float()
        i, gg, f, o = gates.chunk(4, dim=1)
        c_new = torch.sigmoid(f + 1.0) * c + torch.sigmoid(i) * torch.tanh(gg)
        h_new = torch.sigmoid(o) * torch.tanh(c_new)
        outs.append(h_new)
        keep = (~done[:, t]).float().unsqueeze(1)
        h, c = h_new * keep, c_new * keep
    return torch.stack(outs, dim=1), h, c
