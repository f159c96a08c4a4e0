"""finitestateentropy_amd -- MI355X-native block entropy coding (FSE / tANS and Huff0).

The product is the C-ABI shared library ``csrc/libfsehip.so`` (hand-written HIP kernels for gfx950,
declared in ``include/fsehip.h``).  This package is only the thin host-side binding used by the tests and
by ``bench.py``: ctypes calls on raw device pointers, with PyTorch providing device memory, streams and
``torch.distributed``.  There is no CPU fallback: importing :mod:`finitestateentropy_amd.api` raises if the
library has not been built (``python -c 'import __graft_entry__ as g; g.build()'``).
"""
from ._lib import build_library, library_path  # noqa: F401

__all__ = ["build_library", "library_path", "DeltaBase", "SparsePlanes", "tensor_digests"]


def __getattr__(name):
    # DeltaBase (the `base` of compress_tensors with its op, "sub" or "xor", and check=True for a digest of the base), SparsePlanes (its
    # `codec` with the sparse threshold) and tensor_digests (the digests themselves) live in .api, which needs torch and the built library:
    # on first use
    if name in ("DeltaBase", "SparsePlanes", "tensor_digests"):
        from . import api
        return getattr(api, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
