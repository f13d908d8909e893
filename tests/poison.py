"""poisoned(): torch.empty / torch.empty_like / Tensor.new_empty hand back NaN-filled float and sentinel-filled integer
tensors inside the block.  Running a kernel call once plainly and once poisoned, and requiring the same bits, catches
kernels that leave an output element or a workspace slot unwritten and so depend on what the allocator returned."""
import contextlib

import torch

SENTINEL = -0x5A5A5A5A


def _fill(t):
    if t.is_floating_point() or t.is_complex():
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(SENTINEL if t.dtype in (torch.int32, torch.int64) else -1)
    return t


@contextlib.contextmanager
def poisoned():
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    torch.empty = lambda *a, **k: _fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: _fill(empty_like(*a, **k))
    torch.Tensor.new_empty = lambda self, *a, **k: _fill(new_empty(self, *a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty


def same_bits(x, y):
    """Bitwise equality of two tensors (NaN == NaN when the bits match)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.is_floating_point():
        x, y = x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int64), y.contiguous().view(
            torch.int32 if y.element_size() == 4 else torch.int64)
    return bool(torch.equal(x.cpu(), y.cpu()))


def check_unpoisoned(fn, what=""):
    """Calls fn() plainly and poisoned; its result (a tensor or a tuple of tensors / None) must keep its bits."""
    plain = fn()
    with poisoned():
        again = fn()
    plain = plain if isinstance(plain, (tuple, list)) else (plain,)
    again = again if isinstance(again, (tuple, list)) else (again,)
    for i, (p, q) in enumerate(zip(plain, again)):
        if p is None:
            assert q is None, what
            continue
        assert same_bits(p, q), f"{what}: output {i} differs when torch.empty returns NaN / sentinel-filled memory"
    return plain
