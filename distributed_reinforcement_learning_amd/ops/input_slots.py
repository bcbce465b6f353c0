"""Double-buffered static inputs of a captured step (runtime/graphed.py).

Each input field lives twice, as one ``[2, ...]`` tensor. The captured
forward kernels that read such a field take the address of set 0, the
element distance to set 1 and a device slot word, and read the set the word
names (``drla_slot_base``, ops/hip/drla_common.h). The op wrappers find out
here whether a tensor they were handed is set 0 of a registered field: the
same kind of module-level switch as ``conv_op.STASH_INPUTS``, set by
``GraphedImpalaStep`` around its warmup and captures. A tensor that is not
registered gets no slot, and the kernel reads it where it is."""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

SLOT: Optional[torch.Tensor] = None       # int32 [1] on the device
_DIST: Dict[int, int] = {}                # data_ptr of set 0 -> elements
_NAME: Dict[int, str] = {}                # data_ptr of set 0 -> field
_SEEN: set = set()                        # fields some wrapper asked about


def register(slot_word: torch.Tensor, pairs: Dict[str, torch.Tensor]) -> None:
    """pairs: field -> [2, ...] contiguous tensor; views of pairs[k][0] that
    start at its first element are recognised by lookup()."""
    global SLOT
    clear()
    SLOT = slot_word
    for k, t in pairs.items():
        assert t.shape[0] == 2 and t.is_contiguous()
        _DIST[t.data_ptr()] = t[0].numel()
        _NAME[t.data_ptr()] = k


def clear() -> None:
    global SLOT
    SLOT = None
    _DIST.clear()
    _NAME.clear()
    _SEEN.clear()


def unseen() -> list:
    """Registered fields no wrapper has looked up since register(): a field
    listed here is read by something that takes no slot word (it would read
    set 0 whatever the word says)."""
    return sorted(set(_NAME.values()) - _SEEN)


def lookup(t: Optional[torch.Tensor]) -> Tuple[Optional[torch.Tensor], int]:
    """(slot word, element distance) for set 0 of a registered field,
    (None, 0) for anything else."""
    if SLOT is None or t is None:
        return None, 0
    d = _DIST.get(t.data_ptr())
    if d is None:
        return None, 0
    _SEEN.add(_NAME[t.data_ptr()])
    return SLOT, d
