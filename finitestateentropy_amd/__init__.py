"""finitestateentropy_amd -- MI355X-native block entropy coding (FSE / tANS and Huff0).

The product is the C-ABI shared library ``csrc/libfsehip.so`` (hand-written HIP kernels for gfx950,
declared in ``include/fsehip.h``).  This package is only the thin host-side binding used by the tests and
by ``bench.py``: ctypes calls on raw device pointers, with PyTorch providing device memory, streams and
``torch.distributed``.  There is no CPU fallback: importing :mod:`finitestateentropy_amd.api` raises if the
library has not been built (``python -c 'import __graft_entry__ as g; g.build()'``).
"""
from ._lib import build_library, library_path  # noqa: F401

_FROM_API = ("DeltaBase", "SparsePlanes", "PredictedPlanes", "tensor_digests", "archive_tensors", "open_archive", "save_tensors", "load_tensors", "estimate_tensors",
             "compress_tensors_auto", "TensorBundle", "compress_tensors_each", "decompress_tensor_windows_each",
             "patch_tensor_windows_each", "decompress_tensor_windows_each_stride", "patch_tensor_windows_each_stride")
__all__ = ["build_library", "library_path"] + list(_FROM_API)


def __getattr__(name):
    # DeltaBase (the `base` of compress_tensors with its op, "sub" or "xor", and check=True for a digest of the base), SparsePlanes (its
    # `codec` with the sparse threshold), PredictedPlanes (its `codec` with neighbour prediction), tensor_digests (the digests themselves) and the tensor archives (archive_tensors / open_archive: a
    # CompressedTensors as one device buffer and back; save_tensors / load_tensors: the same through a file) live in .api, which needs torch
    # and the built library, as do estimate_tensors / compress_tensors_auto (the plane transform chosen per tensor from device estimates) and the
    # TensorBundle they return, and compress_tensors_each (the same choice without cutting the list: one CompressedTensors with a transform
    # per tensor) and decompress_tensor_windows_each (element windows of such an object, of a predicted one and of a plain or delta one) and
    # patch_tensor_windows_each (the write side of those windows: only the segment frames that hold a window are coded again), and their
    # _stride namesakes, which also take objects that hold a stride above 1: on first use
    if name in _FROM_API:
        from . import api
        return getattr(api, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
