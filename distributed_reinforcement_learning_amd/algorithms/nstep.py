"""n-step returns inside a replayed window, and R2D2 sequence priorities.

The reference math of the fused n-step TD tail (drla_r2d2_nstep_loss_fwd,
ops/hip/r2d2_loss.hip). Pure torch and dtype-preserving, so the tests run
it in float64. For a window of W rows with T1 = W-1 trained positions:

    k      = min(n, T1 - t)                (truncate at the window end)
    Gam_0  = 1,  Gam_{j+1} = Gam_j * disc_{t+j}
    z_t    = sum_{j<k} Gam_j r_{t+j} + Gam_k boot_{t+k}

A zero discount (done) at t+j zeroes every later reward and the bootstrap.
"""

from __future__ import annotations

from typing import Optional

import torch


def nstep_window_target(bootstrap: torch.Tensor, rewards: torch.Tensor,
                        discounts: torch.Tensor, n_step: int) -> torch.Tensor:
    """bootstrap [B,W]: un-rescaled value to bootstrap from AT each row
    (row 0 is never used); rewards [B,W] already clipped; discounts [B,W]
    = 0 where done, gamma elsewhere. Returns z [B,W-1].

    Vectorised as the backward recursion z(m)_t = r_t + disc_t z(m-1)_{t+1}
    with z(0) = bootstrap and the last row pinned to its bootstrap, which
    is what truncates a return that would leave the window."""
    if n_step < 1:
        raise ValueError(f"n_step={n_step} must be >= 1")
    T1 = bootstrap.shape[1] - 1
    r, d = rewards[:, :-1], discounts[:, :-1]
    last = bootstrap[:, -1:]
    z = bootstrap
    for _ in range(min(int(n_step), T1)):
        z = torch.cat([r + d * z[:, 1:], last], dim=1)
    return z[:, :-1]


def sequence_priority(td: torch.Tensor,
                      eta: Optional[float] = None) -> torch.Tensor:
    """td [B,T1] signed -> priority [B]. eta None: |mean_t td| (the TF
    reference's; signed errors cancel). Otherwise the R2D2 paper's
    eta * max_t |td| + (1 - eta) * mean_t |td|, 0 <= eta <= 1."""
    if eta is None:
        return td.mean(dim=1).abs()
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"priority_eta={eta} must be in [0, 1]")
    a = td.abs()
    return eta * a.max(dim=1).values + (1.0 - eta) * a.mean(dim=1)
