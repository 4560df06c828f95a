"""Leaf helpers of the GPU tests (a plain module, like sweep_cases.py): uploads and downloads, bit-for-bit comparison, and output buffers with guard zones.
Addresses and the stream go to the library through api.addr / api.torch_stream."""
import numpy as np
import torch

GUARD, SENTINEL = 64, 77.0


def dev(a, tdt=None):
    """a copying upload (cached inputs are read-only), converted to `tdt` when given; None stays None"""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, order="C"))
    return (t if tdt is None else t.to(tdt)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(a, b):
    """bit for bit (NaN-safe)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same(what, got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert got.tobytes() == ref.tobytes(), (what, int((got != ref).sum()), got.size)


def tdt_of(gm):
    return torch.float32 if gm.dtype_code else torch.float64


def guarded(shape, tdt):
    """an output that starts as NaN (int32: -77), with GUARD elements of SENTINEL in front of it and behind it"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=tdt, device="cuda")
    flat[GUARD:GUARD + n] = -77 if tdt == torch.int32 else float("nan")
    return flat[GUARD:GUARD + n].view(tuple(shape))


def guards_intact(t):
    flat, n = t._base, t.numel()
    assert flat.numel() == n + 2 * GUARD
    return bool((flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all())
