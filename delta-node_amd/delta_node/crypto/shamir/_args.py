"""The argument rules the vector API's methods share, one definition each.

Every rule takes the calling method's name (`what`) where its message carries
it, so that the text a caller sees is the method's own.  A rule lives here
when two or more methods state it in the same words and at the same place in
their order of checks; a check whose text or order is one method's own stays
in that method.  The tensor-list methods test each tensor's usual form inline
(a model's hundred tensors: no call per tensor) and come here only to report
one that failed it.
"""
from __future__ import annotations

import numbers
from typing import List, Optional, Sequence, Tuple


def fits_u64(x: int) -> bool:
    """An abscissa the kernels take: a wire record's x is 64 bits at most."""
    return 0 <= x < (1 << 64)


def check_limits(what: str, threshold: int, shares: int, max_shares: int, max_threshold: int) -> None:
    """make_shares' own check (shamir.py:56-57), then the split kernels' limits."""
    if threshold > shares:
        raise ValueError("threshold should be little equal than shares")
    if shares > max_shares or threshold > max_threshold:
        raise NotImplementedError(f"{what}: at most {max_shares} shares and threshold {max_threshold}")


def check_share_out(what: str, out, shares: int, vb: int, dev) -> None:
    """A caller's share block: contiguous uint8 [shares, vb] on dev."""
    import torch

    if out.dtype != torch.uint8 or tuple(out.shape) != (shares, vb) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{what}: out must be contiguous uint8 [{shares}, {vb}] on {dev}")


def rows_of(block) -> list:
    """The share vectors of one tensor: the rows of a 2-D block, else the sequence's items."""
    import torch

    return list(block.unbind(0)) if isinstance(block, torch.Tensor) and block.dim() == 2 else list(block)


def check_out_form(what: str, out: str) -> None:
    if out not in ("int64", "field"):
        raise ValueError(f'{what}: out must be "int64" or "field"')


def result(out: str, n: int, vb: int, dev) -> tuple:
    """The fresh result of out="int64" | "field" and the (out_fe, out_u64)
    pair that hands it to the reconstruct launches: (res, out_fe, out_u64)."""
    import torch

    if out == "int64":
        res = torch.empty(n, dtype=torch.int64, device=dev)
        return res, None, res
    res = torch.empty(vb, dtype=torch.uint8, device=dev)
    return res, res, None


def wire_pairs(what: str, records) -> List[tuple]:
    recs = [tuple(r) for r in records]
    if any(len(r) != 2 for r in recs):
        raise ValueError(f"{what}: records must be (packed, offsets) pairs")
    return recs


def check_wires(what: str, recs: Sequence[tuple], n: int):
    """A non-empty list of (packed, offsets) wires of n records each: contiguous
    1-D uint8 / int64 tensors on one device, n + 1 offsets.  Returns that device."""
    import torch

    first = recs[0][0]
    for packed, offsets in recs:
        if not (isinstance(packed, torch.Tensor) and packed.dtype == torch.uint8 and packed.dim() == 1
                and packed.is_contiguous()):
            raise ValueError(f"{what}: packed records must be contiguous 1-D uint8 tensors")
        if not (isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int64 and offsets.dim() == 1
                and offsets.is_contiguous()):
            raise ValueError(f"{what}: offsets must be contiguous 1-D int64 tensors")
        if packed.device != first.device or offsets.device != first.device:
            raise ValueError(f"{what}: every wire's records and offsets must be on one device")
        if offsets.numel() < n + 1:
            raise ValueError(f"{what}: offsets must hold n + 1 = {n + 1} entries, got {offsets.numel()}")
    return first.device


def aligned_wires(recs: Sequence[tuple]) -> Tuple[list, list]:
    """The kernels load dwords: one aligned device copy of a misaligned
    `packed` view.  Returns the wires (they own the copies: keep them until
    the launch is queued) and their (address, bytes, offsets address) triples."""
    recs = [(p.clone() if p.data_ptr() & 3 else p, o) for p, o in recs]
    return recs, [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in recs]


def negate_flags(what: str, signs, m: int, noun: str) -> Optional[List[bool]]:
    """`signs` (None, or m values +1 / -1: no bools, no floats) as negate flags."""
    if signs is None:
        return None
    signs = list(signs)
    if len(signs) != m:
        raise ValueError(f"{what}: {len(signs)} signs for {m} {noun}")
    if any(isinstance(s, bool) or not isinstance(s, numbers.Integral) or s not in (1, -1) for s in signs):
        raise ValueError(f"{what}: signs must be +1 or -1")
    return [s < 0 for s in signs]


def check_bad_flag(what: str, bad, dev, noun: str) -> None:
    """A caller's deferred-error flag: None, or int32 [2] on the `noun`s' device."""
    import torch

    if bad is not None and not (isinstance(bad, torch.Tensor) and bad.dtype == torch.int32
                                and tuple(bad.shape) == (2,) and bad.is_contiguous() and bad.device == dev):
        raise ValueError(f"{what}: bad must be a contiguous int32 tensor [2] on the {noun}' device")


def bad_flag(bad, dev) -> tuple:
    """(flag, checked): the caller's flag, or a zeroed one of this call's own
    that the call reads back and raises from once its launches are queued."""
    import torch

    if bad is None:
        return torch.zeros(2, dtype=torch.int32, device=dev), True
    return bad, False
