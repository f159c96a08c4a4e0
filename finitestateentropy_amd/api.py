"""Host-side mirror of the reference block API (lib/fse.h, lib/huf.h, lib/hist.h) over libfsehip.so.

Batched functions take / return CUDA (HIP) ``torch.uint8`` tensors and call the C ABI with raw device
pointers on torch's current stream.  ``results`` tensors are ``torch.int64`` views of the reference's
``size_t`` return values: a negative value ``-c`` is the error code ``c`` of lib/error_public.h:45-56.
Single-block functions take numpy arrays (host pointers) and have the reference's exact signatures.
"""
import contextlib
import ctypes as C
import json
import numbers

import numpy as np
import torch

from . import _lib

SZ = C.c_size_t
VP = C.c_void_p

ERROR_NAMES = {1: "GENERIC", 2: "dstSize_tooSmall", 3: "srcSize_wrong", 4: "corruption_detected", 5: "tableLog_tooLarge",
               6: "maxSymbolValue_tooLarge", 7: "maxSymbolValue_tooSmall", 8: "workSpace_tooSmall"}


CODECS_GIVEN, CODECS_CHOOSE = 0, 1      # FSEHIP_CODECS_GIVEN / FSEHIP_CODECS_CHOOSE (include/fsehip.h)


class AutoCodec:
    """`codec` of compress_tensors: a codec per frame, chosen by size on the device -- Huff0 unless its frame is more than
    tolerance_permille / 1000 larger than the FSE frame (FSEHIP_CODECS_CHOOSE, include/fsehip.h)."""

    def __init__(self, tolerance_permille=0):
        if not isinstance(tolerance_permille, numbers.Integral) or not 0 <= tolerance_permille <= 1000:
            raise ValueError("tolerance_permille %r: 0 .. 1000" % (tolerance_permille,))
        self.tolerance_permille = int(tolerance_permille)

    def __repr__(self):
        return "AutoCodec(%d)" % self.tolerance_permille

    def __eq__(self, other):
        return isinstance(other, AutoCodec) and other.tolerance_permille == self.tolerance_permille

    def __hash__(self):
        return hash(("AutoCodec", self.tolerance_permille))


class SparsePlanes:
    """`codec` of compress_tensors and compress_tensors_segmented: the planes (segments) go to the frame writers as SPARSE contents -- a zero
    mask of one bit per byte and the non-zero bytes -- wherever at most permille / 1000 of a plane's bytes are non-zero and that form is
    shorter (include/fsehip.h "sparse planes").  `codec` is what codes the contents: 0 (FSE), 1 (Huff0) or an AutoCodec.  The reason is the
    sign / exponent plane of a tensor delta, almost all zeros: as a sparse content its Huff0 frame shrinks from 33 KB to under 5 KB per
    256 KB, and FSE has a fraction of the symbols to decode.  The object written carries `sparse_permille`; decompress_tensors reads it."""

    def __init__(self, codec=0, permille=500):
        if not isinstance(codec, AutoCodec) and (isinstance(codec, bool) or codec not in (0, 1)):
            raise ValueError("SparsePlanes: codec %r, 0 (FSE), 1 (Huff0) or an AutoCodec is needed" % (codec,))
        if not isinstance(permille, numbers.Integral) or isinstance(permille, bool) or not 0 <= permille <= 1000:
            raise ValueError("SparsePlanes: permille %r, 0 .. 1000 is needed" % (permille,))
        self.codec, self.permille = codec if isinstance(codec, AutoCodec) else int(codec), int(permille)

    def __repr__(self):
        return "SparsePlanes(%r, %d)" % (self.codec, self.permille)

    def __eq__(self, other):
        return isinstance(other, SparsePlanes) and other.codec == self.codec and other.permille == self.permille

    def __hash__(self):
        return hash(("SparsePlanes", self.codec, self.permille))


class PredictedPlanes:
    """`codec` of compress_tensors and compress_tensors_segmented: the planes are those of zigzag(element - the element in front of it), the
    elements taken as unsigned integers and the predecessor as 0 at the start of every run of 1024 elements (include/fsehip.h "predicted
    planes").  `codec` is what codes them: 0 (FSE), 1 (Huff0) or an AutoCodec.  For tensors whose neighbours are close -- sorted indices,
    offsets, position ids, sampled fields, audio; weights get worse.  Opt-in, never chosen automatically.  The object written carries
    `predictor` ("prev"); decompress_tensors reads it.  Not combined with a base or with SparsePlanes; windows and patches of a
    segmented object: decompress_tensor_windows_each and patch_tensor_windows_each.
    `stride` (1 .. 8, include/fsehip.h "strided predicted planes"): the predecessor is the element `stride` elements in front -- the same
    channel of interleaved data: 2 for stereo samples or complex pairs, 3 for RGB or xyz, 4 for RGBA or boxes -- and 0 for the first
    `stride` elements of every run.  The object then carries the predictor "prev<stride>" ("prev3"); windows and patches of such a
    segmented object: decompress_tensor_windows_each_stride and patch_tensor_windows_each_stride (the calls without _stride refuse it)."""

    def __init__(self, codec=0, stride=1):
        if not isinstance(codec, AutoCodec) and (isinstance(codec, (bool, SparsePlanes, PredictedPlanes)) or codec not in (0, 1)):
            raise ValueError("PredictedPlanes: codec %r, 0 (FSE), 1 (Huff0) or an AutoCodec is needed" % (codec,))
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= PRED_MAX_STRIDE:
            raise ValueError("PredictedPlanes: stride %r, an integer 1 .. %d is needed" % (stride, PRED_MAX_STRIDE))
        self.codec = codec if isinstance(codec, AutoCodec) else int(codec)
        self.stride = int(stride)

    @property
    def predictor(self):
        return predictor_name(self.stride)

    def __repr__(self):
        return "PredictedPlanes(%r)" % (self.codec,) if self.stride == 1 else "PredictedPlanes(%r, stride=%d)" % (self.codec, self.stride)

    def __eq__(self, other):
        return isinstance(other, PredictedPlanes) and other.codec == self.codec and other.stride == self.stride

    def __hash__(self):
        return hash(("PredictedPlanes", self.codec, self.stride))


PRED_MAX_STRIDE = 8                     # FSEHIP_PRED_MAX_STRIDE (include/fsehip.h)


def predictor_name(stride):
    """the `predictor` of an object written with PredictedPlanes(codec, stride): "prev" for stride 1, "prev<stride>" above"""
    return "prev" if stride == 1 else "prev%d" % stride


def predictor_stride(predictor, what):
    """the stride behind an object's `predictor`: "prev" -> 1, "prev2" .. "prev8" -> 2 .. 8; anything else ("prev0", "prev1", "prev9",
    "next") is a ValueError -- a reader that does not know a predictor refuses it and never decodes wrongly"""
    if predictor == "prev":
        return 1
    if isinstance(predictor, str) and len(predictor) == 5 and predictor.startswith("prev") and predictor[4] in "2345678":
        return int(predictor[4])
    raise ValueError("%s: predictor %r; \"prev\" and \"prev2\" .. \"prev%d\" are the ones there are" % (what, predictor, PRED_MAX_STRIDE))


DELTA_OPS = {"xor": 0, "sub": 1}        # FSEHIP_DELTA_XOR / FSEHIP_DELTA_SUB (include/fsehip.h)


class DeltaBase:
    """`base` of compress_tensors with the delta's operation beside it: "sub" -- the elements' bit patterns subtracted as integers and
    zigzag-folded (FSEHIP_DELTA_SUB, include/fsehip.h "arithmetic tensor deltas"), 11 to 19 % fewer frame bytes than XOR on weight updates
    -- or "xor", which is what a plain sequence as `base` means.  The object written carries the op as `delta_op`; the reading calls take
    the op from the object and the base as a plain sequence, or as a DeltaBase of the same op.
    check=True: the writing call digests the base tensors on the device (include/fsehip.h "tensor digests and checked deltas") and the
    object carries them as `base_digests`; decompress_tensors then digests the base it is given and refuses (ValueError, nothing written)
    a base that is not the one the deltas were made against.  The digest is not cryptographic: it catches accidents, not adversaries."""

    def __init__(self, tensors, op="sub", check=False):
        if not isinstance(op, str) or op not in DELTA_OPS:
            raise ValueError("DeltaBase: op %r, \"sub\" or \"xor\" is needed" % (op,))
        if not isinstance(check, bool):
            raise ValueError("DeltaBase: check %r, True or False is needed" % (check,))
        self.tensors, self.op, self.check = list(tensors), op, check

    def __len__(self):
        return len(self.tensors)

    def __iter__(self):
        return iter(self.tensors)

    def __repr__(self):
        return "DeltaBase(%d tensors, op=%r%s)" % (len(self.tensors), self.op, ", check=True" if self.check else "")


def fse_compress_bound(n):      # lib/fse.h:290-292
    return 512 + n + (n >> 7) + 4 + 8


def huf_compress_bound(n):      # lib/huf.h:131-133
    return 129 + n + (n >> 8) + 8


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: hipError %d" % (what, rc))


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def _sizes_arg(sizes, like=None):
    """sizes: None | integer (python or numpy) | integer cuda tensor -> (device pointer or NULL, uniform, keepalive)"""
    if sizes is None or isinstance(sizes, numbers.Integral):
        return VP(0), SZ(int(sizes or 0)), None
    if not isinstance(sizes, torch.Tensor) or not sizes.is_cuda:
        raise TypeError("per-block sizes must be an integer or a CUDA integer tensor (the C ABI takes a device pointer)")
    if like is not None and sizes.device != like.device:
        raise ValueError("sizes live on %s, the blocks on %s" % (sizes.device, like.device))
    t = sizes.to(torch.int64).contiguous()
    return VP(t.data_ptr()), SZ(0), t


def _blocks(t, what):
    """a batch of byte blocks handed to the C ABI as (base pointer, row stride): uint8, on the GPU, rows contiguous"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2:
        raise TypeError("%s must be a 2-D CUDA uint8 tensor" % what)
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError("%s: bytes of a block must be contiguous (stride(1) == 1); call .contiguous()" % what)
    return t


class _Guarded:
    """Destination of a batched call in guard mode (FseHip.guard > 0): every block's slot is followed by `guard` bytes of 0xA5 -- the
    row stride is capacity + guard, the capacity handed to the library stays `cap` -- and `check()` asserts after the call that no
    kernel touched them: the device-side form of the reference fuzzers' guard byte (programs/fuzzer.c:217-230,
    programs/fuzzerHuff0.c:198-212; SURVEY 8(b): nothing is written beyond dst + dstCapacity)."""
    FILL = 0xA5

    def __init__(self, n, cap, guard, device, dtype=torch.uint8, zero=False):
        self.cap = cap
        self.full = torch.empty((n, max(cap, 1) + guard), dtype=dtype, device=device)
        self.fill = self.FILL if dtype == torch.uint8 else 0xA5A5 - 0x10000
        self.full.fill_(self.fill)
        self.view = self.full[:, :max(cap, 1)]
        if zero and cap > 0:
            self.view.zero_()

    def check(self, what, sizes=None):
        """sizes: per-block capacities (tensor) when they differ from block to block (Huff0 decoders: the exact regenerated size)"""
        if sizes is None or isinstance(sizes, numbers.Integral):
            cap = self.cap if sizes is None else int(sizes)
            touched = self.full[:, cap:] != self.fill
            caps = None
        else:
            caps = sizes.to(torch.int64).to(self.full.device).clamp(max=self.full.shape[1])
            cols = torch.arange(self.full.shape[1], device=self.full.device)
            touched = (self.full != self.fill) & (cols[None, :] >= caps[:, None])
            cap = 0
        bad = touched.any(dim=1)
        if bool(bad.any().item()):
            rows = torch.nonzero(bad).flatten()[:8].tolist()
            b = rows[0]
            where = (torch.nonzero(touched[b]).flatten()[:8] + cap).tolist()
            raise AssertionError("%s wrote past its destination capacity (%s): blocks %s (block %d at byte offsets %s)"
                                 % (what, self.cap if caps is None else int(caps[b]), rows, b, where))


class FseHip:
    # > 0: the batch helpers below that allocate their own destination put `guard` sentinel bytes (symbols for the 16-bit coder)
    # behind every block's capacity and assert after the call that they are untouched (synchronises; tests only)
    guard = 0

    def _dst(self, n, cap, device, zero=False, dtype=torch.uint8):
        """(destination tensor handed to the library, guard object or None)"""
        if self.guard > 0:
            g = _Guarded(n, cap, self.guard, device, dtype, zero)
            return g.view, g
        alloc = torch.zeros if zero else torch.empty
        return alloc((n, max(cap, 1)), dtype=dtype, device=device), None

    def __init__(self):
        self.lib = _lib.load()
        L = self.lib
        for name in ("FSEHIP_HIST_count", "FSEHIP_FSE_compress_usingCTable", "FSEHIP_FSE_decompress_usingDTable",
                     "FSEHIP_FSE_compress", "FSEHIP_FSE_compress2", "FSEHIP_FSE_decompress",
                     "FSEHIP_HUF_compress1X_usingCTable", "FSEHIP_HUF_compress4X_usingCTable",
                     "FSEHIP_HUF_decompress4X_usingDTable", "FSEHIP_HUF_decompress4X1_usingDTable",
                     "FSEHIP_HUF_decompress1X_usingDTable", "FSEHIP_HUF_decompress1X1_usingDTable",
                     "FSEHIP_HUF_compress", "FSEHIP_HUF_compress2", "FSEHIP_HUF_decompress",
                     "FSEHIP_FSE_compress_batch_workspaceSize", "FSEHIP_FSE_decompress_batch_workspaceSize",
                     "FSEHIP_HUF_compress_batch_workspaceSize", "FSEHIP_HUF_decompress_batch_workspaceSize",
                     "FSEHIP_frame_compressBound", "FSEHIP_frame_compress", "FSEHIP_frame_decompress", "FSEHIP_frame_compress_batch", "FSEHIP_frame_decompress_batch",
                     "FSEHIP_FSE_countU16", "FSEHIP_FSE_compressU16", "FSEHIP_FSE_decompressU16",
                     "FSEHIP_FSE_compressU16_batch_workspaceSize", "FSEHIP_FSE_decompressU16_batch_workspaceSize",
                     "FSEHIP_FSE_buildCTable_batch_workspaceSize", "FSEHIP_FSE_buildDTable_batch_workspaceSize",
                     "FSEHIP_HUF_buildCTable_batch_workspaceSize", "FSEHIP_HUF_readDTableX1_batch_workspaceSize", "FSEHIP_HUF_readDTableX2_batch_workspaceSize",
                     "FSEHIP_compact_batch_workspaceSize", "FSEHIP_compact_batch_bound", "FSEHIP_HUF_compress1X",
                     "FSEHIP_HUF_decompress4X1", "FSEHIP_HUF_decompress1X1"):
            if hasattr(L, name):
                getattr(L, name).restype = SZ
        L.FSEHIP_getErrorName.restype = C.c_char_p
        L.FSEHIP_versionString.restype = C.c_char_p

    # ------------------------------------------------------------------ info
    def device_info(self):
        class Info(C.Structure):
            _fields_ = [("deviceOrdinal", C.c_int), ("computeUnits", C.c_int), ("ldsBytesPerCU", C.c_int),
                        ("wavefrontSize", C.c_int), ("archName", C.c_char * 64)]
        info = Info()
        _check(self.lib.FSEHIP_deviceInfo(C.byref(info)), "deviceInfo")
        return {"device": info.deviceOrdinal, "cus": info.computeUnits, "lds_per_cu": info.ldsBytesPerCU,
                "wave": info.wavefrontSize, "arch": info.archName.decode()}

    # ------------------------------------------------------------------ workload
    def probagen_table(self, p):
        t = np.zeros(4096, dtype=np.uint8)
        self.lib.FSEHIP_probagen_table(t.ctypes.data_as(VP), C.c_double(p))
        return t

    def probagen_batch(self, p_percent, n_blocks, block_size=32768, first_seed=1, out=None, device="cuda", seed_step=1):
        """block b = probagen(block_size, p, seed=first_seed + b*seed_step)  (programs/probaGenerator.c)"""
        table = self.probagen_table(p_percent / 100.0)
        if out is None:
            out = torch.empty((n_blocks, block_size), dtype=torch.uint8, device=device)
        _check(self.lib.FSEHIP_probagen_batch_ex(_ptr(out), SZ(out.stride(0)), SZ(block_size), SZ(n_blocks),
                                                 table.ctypes.data_as(VP), C.c_uint32(first_seed & 0xFFFFFFFF), C.c_uint32(seed_step), _stream()), "probagen_batch")
        return out

    def probagen_mixed(self, probas, n_blocks, block_size=32768, first_block=0, device="cuda", out=None):
        """BASELINE config 5 corpus: global block g (= first_block + row) is drawn from distribution probas[g mod len(probas)]
        with seed g + 1 -- one strided generator call per distribution (into `out` if given)."""
        if out is None:
            out = torch.empty((n_blocks, block_size), dtype=torch.uint8, device=device)
        k = len(probas)
        for j in range(k):
            r0 = (j - first_block) % k                       # first row whose global index is congruent to j
            rows = out[r0::k]
            if rows.shape[0]:
                self.probagen_batch(probas[j], rows.shape[0], block_size, first_seed=first_block + r0 + 1, out=rows, seed_step=k)
        return out

    # ------------------------------------------------------------------ a1
    def hist_count_batch(self, src, sizes=None, max_symbol_values=None):
        n = _blocks(src, "src").shape[0]
        counts = torch.zeros((n, 256), dtype=torch.int32, device=src.device)
        msv = (torch.full((n,), 255, dtype=torch.int32, device=src.device) if max_symbol_values is None
               else max_symbol_values.to(torch.int32).contiguous().clone())
        res = torch.zeros(n, dtype=torch.int64, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_HIST_count_batch(_ptr(counts), _ptr(msv), _ptr(res), _ptr(src), SZ(src.stride(0)), ps, uni,
                                                SZ(n), _stream()), "HIST_count_batch")
        return counts, msv, res

    # ------------------------------------------------------------------ a2 / a3
    def fse_compress_using_ctable_batch(self, src, ctables, max_table_log=12, sizes=None, dst_capacity=None, shared_table=False, dst=None, results=None):
        n = _blocks(src, "src").shape[0]
        cap = fse_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=src.device) if results is None else results
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        stride = 0 if shared_table else ctables.stride(0)
        _check(self.lib.FSEHIP_FSE_compress_usingCTable_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(res), _ptr(src), SZ(src.stride(0)),
                                                              ps, uni, _ptr(ctables), SZ(stride), C.c_uint(max_table_log), SZ(n), _stream()),
               "FSE_compress_usingCTable_batch")
        if g:
            g.check("FSE_compress_usingCTable_batch")
        return dst, res

    def fse_decompress_using_dtable_batch(self, csrc, csizes, dtables, dst_capacity, max_table_log=12, shared_table=False, dst=None, results=None):
        n = _blocks(csrc, "csrc").shape[0]
        g = None
        if dst is None:
            dst, g = self._dst(n, dst_capacity, csrc.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=csrc.device) if results is None else results
        ps, uni, keep = _sizes_arg(csizes, csrc)
        stride = 0 if shared_table else dtables.stride(0)
        _check(self.lib.FSEHIP_FSE_decompress_usingDTable_batch(_ptr(dst), SZ(dst.stride(0)), SZ(dst_capacity), _ptr(res), _ptr(csrc),
                                                                SZ(csrc.stride(0)), ps, uni, _ptr(dtables), SZ(stride),
                                                                C.c_uint(max_table_log), SZ(n), _stream()),
               "FSE_decompress_usingDTable_batch")
        if g:
            g.check("FSE_decompress_usingDTable_batch")
        return dst, res

    # ------------------------------------------------------------------ one-shot FSE over a batch
    def fse_workspace(self, n_blocks, table_log=11, decompress=False, device="cuda"):
        fn = self.lib.FSEHIP_FSE_decompress_batch_workspaceSize if decompress else self.lib.FSEHIP_FSE_compress_batch_workspaceSize
        nbytes = int(fn(SZ(n_blocks), C.c_uint(table_log)))
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def fse_compress_batch(self, src, table_log=11, max_symbol_value=255, sizes=None, dst=None, dst_capacity=None, results=None, workspace=None):
        n = _blocks(src, "src").shape[0]
        cap = (fse_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity)
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=src.device)
        if workspace is None:
            workspace = self.fse_workspace(n, table_log, False, src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_FSE_compress_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(results), _ptr(src), SZ(src.stride(0)), ps, uni,
                                                  C.c_uint(max_symbol_value), C.c_uint(table_log), SZ(n), _ptr(workspace),
                                                  SZ(workspace.numel()), _stream()), "FSE_compress_batch")
        if g:
            g.check("FSE_compress_batch")
        return dst, results

    def fse_decompress_batch(self, csrc, csizes, dst_capacity, max_log=12, dst=None, results=None, workspace=None):
        n = _blocks(csrc, "csrc").shape[0]
        g = None
        if dst is None:
            dst, g = self._dst(n, dst_capacity, csrc.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=csrc.device)
        if workspace is None:
            workspace = self.fse_workspace(n, max_log, True, csrc.device)
        ps, uni, keep = _sizes_arg(csizes, csrc)
        _check(self.lib.FSEHIP_FSE_decompress_batch(_ptr(dst), SZ(dst.stride(0)), SZ(dst_capacity), _ptr(results), _ptr(csrc), SZ(csrc.stride(0)),
                                                    ps, uni, C.c_uint(max_log), SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()),
               "FSE_decompress_batch")
        if g:
            g.check("FSE_decompress_batch")
        return dst, results

    @contextlib.contextmanager
    def decode_timing(self):
        """Between entry and exit the bit-reversed classes of both FSE decoders run through the TIMED instantiation of k_fse_decode
        (FSEHIP_debug_decodeTiming, csrc/fse_decode.hip).  Yields a list that holds the 16 counters of g_decTiming once the block has been
        left -- [2] rounds that ran a long phase, [10] rounds of finishing phases, [4] decoder waves that went through the bulk.  The switch
        is process-wide and goes back off whatever happens inside; both ends synchronise the device.  A measurement and test aid."""
        out = []
        _check(self.lib.FSEHIP_debug_decodeTiming(1, None), "debug_decodeTiming(1)")
        buf = (C.c_ulonglong * 16)()
        try:
            yield out
        finally:
            _check(self.lib.FSEHIP_debug_decodeTiming(0, buf), "debug_decodeTiming(0)")
            out.extend(int(v) for v in buf)

    # ------------------------------------------------------------------ tables built on the device (g1-g3)
    def fse_build_ctable_batch(self, src, table_log=11, max_symbol_value=255, sizes=None, header_capacity=512, ctables=None):
        """FSE_buildCTable_batch: (ctables (n, FSE_CTABLE_SIZE_U32(max(table_log, 9), 255)) int32, headers (n, header_capacity) uint8, results)"""
        n = _blocks(src, "src").shape[0]
        tl = min(max(table_log or 11, 9), 12)
        ctw = 1 + (1 << (tl - 1)) + 512
        ct = torch.zeros((n, ctw), dtype=torch.int32, device=src.device) if ctables is None else ctables
        hdr, g = self._dst(n, header_capacity, src.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=src.device)
        ws = torch.empty(int(self.lib.FSEHIP_FSE_buildCTable_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_FSE_buildCTable_batch(_ptr(ct), SZ(ct.stride(0)), _ptr(hdr), SZ(hdr.stride(0)), SZ(header_capacity), _ptr(res), _ptr(src),
                                                     SZ(src.stride(0)), ps, uni, C.c_uint(max_symbol_value), C.c_uint(table_log), SZ(n), _ptr(ws),
                                                     SZ(ws.numel()), _stream()), "FSE_buildCTable_batch")
        if g:
            g.check("FSE_buildCTable_batch")
        return ct, hdr, res

    def fse_build_dtable_batch(self, headers, header_sizes, max_log=12):
        """FSE_buildDTable_batch: (dtables (n, FSE_DTABLE_SIZE_U32(max_log)) int32 in the reference layout, results = header bytes or error)"""
        n = _blocks(headers, "headers").shape[0]
        dt = torch.zeros((n, 1 + (1 << max_log)), dtype=torch.int32, device=headers.device)
        res = torch.zeros(n, dtype=torch.int64, device=headers.device)
        ws = torch.empty(int(self.lib.FSEHIP_FSE_buildDTable_batch_workspaceSize(SZ(n), C.c_uint(max_log))), dtype=torch.uint8, device=headers.device)
        ps, uni, keep = _sizes_arg(header_sizes, headers)
        _check(self.lib.FSEHIP_FSE_buildDTable_batch(_ptr(dt), SZ(dt.stride(0)), _ptr(res), _ptr(headers), SZ(headers.stride(0)), ps, uni,
                                                     C.c_uint(max_log), SZ(n), _ptr(ws), SZ(ws.numel()), _stream()), "FSE_buildDTable_batch")
        return dt, res

    # ------------------------------------------------------------------ table glue, step by step (lib/fse.h:137-156, 222-229)
    def fse_normalize_count_batch(self, counts, totals, max_symbol_values, table_log):
        """FSE_normalizeCount per row of `counts` (n, 256) int32: (norms (n, 256) int16, results = tableLog or error)"""
        n = counts.shape[0]
        norms = torch.zeros((n, 256), dtype=torch.int16, device=counts.device)
        res = torch.zeros(n, dtype=torch.int64, device=counts.device)
        _check(self.lib.FSEHIP_FSE_normalizeCount_batch(_ptr(norms), SZ(256), C.c_uint(table_log), _ptr(counts), SZ(counts.stride(0)), _ptr(totals),
                                                        _ptr(max_symbol_values), SZ(n), _ptr(res), _stream()), "FSE_normalizeCount_batch")
        return norms, res

    def fse_write_ncount_batch(self, norms, max_symbol_values, table_log, capacity=512, stride=None):
        """FSE_writeNCount per row of `norms` (n, 256) int16: (headers (n, stride) uint8 pre-filled with 0xA5, results = header bytes or error)"""
        n = norms.shape[0]
        hdr = torch.full((n, stride or max(capacity, 1)), 0xA5, dtype=torch.uint8, device=norms.device)
        res = torch.zeros(n, dtype=torch.int64, device=norms.device)
        _check(self.lib.FSEHIP_FSE_writeNCount_batch(_ptr(hdr), SZ(hdr.stride(0)), SZ(capacity), _ptr(norms), SZ(norms.stride(0)), _ptr(max_symbol_values),
                                                     C.c_uint(table_log), SZ(n), _ptr(res), _stream()), "FSE_writeNCount_batch")
        return hdr, res

    def fse_read_ncount_batch(self, headers, header_sizes, max_symbol_values):
        """FSE_readNCount per row: (norms (n, 256) int16, maxSymbolValues out, tableLogs, results = bytes read or error)"""
        n = _blocks(headers, "headers").shape[0]
        norms = torch.zeros((n, 256), dtype=torch.int16, device=headers.device)
        msv = max_symbol_values.clone()
        tls = torch.zeros(n, dtype=torch.int32, device=headers.device)
        res = torch.zeros(n, dtype=torch.int64, device=headers.device)
        ps, uni, keep = _sizes_arg(header_sizes, headers)
        _check(self.lib.FSEHIP_FSE_readNCount_batch(_ptr(norms), SZ(256), _ptr(msv), _ptr(tls), _ptr(headers), SZ(headers.stride(0)), ps, uni, SZ(n), _ptr(res),
                                                    _stream()), "FSE_readNCount_batch")
        return norms, msv, tls, res

    def fse_build_ctable_from_norm_batch(self, norms, max_symbol_values, table_log):
        """FSE_buildCTable per row of `norms` (n, 256) int16: (ctables (n, FSE_CTABLE_SIZE_U32(table_log, 255)) int32, results = 0 or error)"""
        n = norms.shape[0]
        ct = torch.zeros((n, 1 + (1 << max(min(table_log, 12) - 1, 0)) + 512), dtype=torch.int32, device=norms.device)
        res = torch.zeros(n, dtype=torch.int64, device=norms.device)
        _check(self.lib.FSEHIP_FSE_buildCTable_fromNorm_batch(_ptr(ct), SZ(ct.stride(0)), _ptr(norms), SZ(norms.stride(0)), _ptr(max_symbol_values),
                                                              C.c_uint(table_log), SZ(n), _ptr(res), _stream()), "FSE_buildCTable_fromNorm_batch")
        return ct, res

    def fse_build_dtable_from_norm_batch(self, norms, max_symbol_values, table_log):
        """FSE_buildDTable per row of `norms` (n, 256) int16: (dtables (n, FSE_DTABLE_SIZE_U32(table_log)) int32, results = 0 or error)"""
        n = norms.shape[0]
        dt = torch.zeros((n, 1 + (1 << max(min(table_log, 12), 1))), dtype=torch.int32, device=norms.device)
        res = torch.zeros(n, dtype=torch.int64, device=norms.device)
        self.lib.FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize.restype = SZ
        ws = torch.empty(int(self.lib.FSEHIP_FSE_buildDTable_fromNorm_batch_workspaceSize(SZ(n), C.c_uint(table_log))), dtype=torch.uint8, device=norms.device)
        _check(self.lib.FSEHIP_FSE_buildDTable_fromNorm_batch(_ptr(dt), SZ(dt.stride(0)), _ptr(norms), SZ(norms.stride(0)), _ptr(max_symbol_values),
                                                              C.c_uint(table_log), SZ(n), _ptr(res), _ptr(ws), SZ(ws.numel()), _stream()), "FSE_buildDTable_fromNorm_batch")
        return dt, res

    # ------------------------------------------------------------------ packed (variable-length) batches
    def compact_batch(self, slots, results, src, sizes=None, packed=None, offsets=None):
        """FSEHIP_compact_batch: (packed uint8 (capacity,), offsets int64 (n + 1,)); offsets[n] = the packed size"""
        n = _blocks(slots, "slots").shape[0]
        _blocks(src, "src")
        if packed is None:
            packed = torch.empty(max(n * src.shape[1], 1), dtype=torch.uint8, device=src.device)
        if offsets is None:
            offsets = torch.empty(n + 1, dtype=torch.int64, device=src.device)
        self.lib.FSEHIP_compact_batch_workspaceSize.restype = SZ
        ws = torch.empty(int(self.lib.FSEHIP_compact_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_compact_batch(_ptr(packed), SZ(packed.numel()), _ptr(offsets), _ptr(slots), SZ(slots.stride(0)), _ptr(results),
                                             _ptr(src), SZ(src.stride(0)), ps, uni, SZ(n), _ptr(ws), SZ(ws.numel()), _stream()), "compact_batch")
        return packed, offsets

    def fse_decompress_packed_batch(self, packed, offsets, orig_sizes, dst_capacity, max_log=12, dst=None, results=None, workspace=None):
        n = offsets.numel() - 1
        g = None
        if dst is None:
            dst, g = self._dst(n, dst_capacity, packed.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=packed.device)
        if workspace is None:
            workspace = self.fse_workspace(n, max_log, True, packed.device)
        po, uo, keep = _sizes_arg(orig_sizes, packed)
        _check(self.lib.FSEHIP_FSE_decompress_packed_batch(_ptr(dst), SZ(dst.stride(0)), SZ(dst_capacity), _ptr(results), _ptr(packed), _ptr(offsets), po, uo,
                                                           C.c_uint(max_log), SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()), "FSE_decompress_packed_batch")
        if g:
            g.check("FSE_decompress_packed_batch")
        return dst, results

    # ------------------------------------------------------------------ layer 1 (host pointers, reference signatures)
    def _single(self, fname, cap, src, *extra):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        out = np.zeros(max(cap, 1) + 16, dtype=np.uint8)
        out[cap:] = 0xA5
        r = int(getattr(self.lib, fname)(out.ctypes.data_as(VP), SZ(cap), src.ctypes.data_as(VP), SZ(src.size), *extra))
        assert (out[cap:] == 0xA5).all(), "%s wrote past dstCapacity" % fname
        return r, out[:cap]

    def hist_count(self, src, max_sv=255):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        count = np.zeros(256, dtype=np.uint32)
        msv = C.c_uint(max_sv)
        r = int(self.lib.FSEHIP_HIST_count(count.ctypes.data_as(VP), C.byref(msv), src.ctypes.data_as(VP), SZ(src.size)))
        return r, int(msv.value), count

    def fse_compress_using_ctable(self, src, ct, cap=None):
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        return self._single("FSEHIP_FSE_compress_usingCTable", fse_compress_bound(len(src)) if cap is None else cap, src, ct.ctypes.data_as(VP))

    def fse_decompress_using_dtable(self, csrc, dt, cap):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        return self._single("FSEHIP_FSE_decompress_usingDTable", cap, csrc, dt.ctypes.data_as(VP))

    # the table glue on host pointers (lib/fse.h:119-163, :222-241): same argument order as the reference, numpy in / out
    def fse_optimal_tablelog(self, max_tl, src_size, max_sv):
        self.lib.FSEHIP_FSE_optimalTableLog.restype = C.c_uint
        return int(self.lib.FSEHIP_FSE_optimalTableLog(C.c_uint(max_tl), SZ(src_size), C.c_uint(max_sv)))

    def fse_ncount_write_bound(self, max_sv, table_log):
        self.lib.FSEHIP_FSE_NCountWriteBound.restype = SZ
        return int(self.lib.FSEHIP_FSE_NCountWriteBound(C.c_uint(max_sv), C.c_uint(table_log)))

    def fse_normalize_count(self, table_log, count, total, max_sv):
        count = np.ascontiguousarray(count, dtype=np.uint32)
        norm = np.full(max(256, max_sv + 1) + 4, 0x5A5A, dtype=np.int16)
        self.lib.FSEHIP_FSE_normalizeCount.restype = SZ
        r = int(self.lib.FSEHIP_FSE_normalizeCount(norm.ctypes.data_as(VP), C.c_uint(table_log), count.ctypes.data_as(VP), SZ(total), C.c_uint(max_sv)))
        assert (norm[max(max_sv, 0) + 1:] == 0x5A5A).all() or max_sv > 255, "FSE_normalizeCount wrote past normalizedCounter[maxSymbolValue]"
        return r, norm[:256]

    def fse_write_ncount(self, cap, norm, max_sv, table_log):
        norm = np.ascontiguousarray(norm, dtype=np.int16)
        out = np.full(max(cap, 1) + 8, 0xA5, dtype=np.uint8)
        self.lib.FSEHIP_FSE_writeNCount.restype = SZ
        r = int(self.lib.FSEHIP_FSE_writeNCount(out.ctypes.data_as(VP), SZ(cap), norm.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(table_log)))
        assert (out[cap:] == 0xA5).all(), "FSE_writeNCount wrote past bufferSize"
        return r, out[:cap]

    def fse_read_ncount(self, src, max_sv=255):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        norm = np.zeros(max(256, max_sv + 1), dtype=np.int16)
        msv, tl = C.c_uint(max_sv), C.c_uint(0)
        self.lib.FSEHIP_FSE_readNCount.restype = SZ
        r = int(self.lib.FSEHIP_FSE_readNCount(norm.ctypes.data_as(VP), C.byref(msv), C.byref(tl), src.ctypes.data_as(VP), SZ(src.size)))
        return r, int(msv.value), int(tl.value), norm

    def fse_build_ctable(self, norm, max_sv, table_log, wksp_bytes=None):
        norm = np.ascontiguousarray(norm, dtype=np.int16)
        words = 1 + (1 << max(min(table_log, 12) - 1, 0)) + 2 * (min(max_sv, 255) + 1)
        ct = np.zeros(words + 4, dtype=np.uint32)
        ct[words:] = 0xA5A5A5A5
        if wksp_bytes is None:
            self.lib.FSEHIP_FSE_buildCTable.restype = SZ
            r = int(self.lib.FSEHIP_FSE_buildCTable(ct.ctypes.data_as(VP), norm.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(table_log)))
        else:
            ws = np.zeros(max(wksp_bytes, 1), dtype=np.uint8)
            self.lib.FSEHIP_FSE_buildCTable_wksp.restype = SZ
            r = int(self.lib.FSEHIP_FSE_buildCTable_wksp(ct.ctypes.data_as(VP), norm.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(table_log), ws.ctypes.data_as(VP), SZ(wksp_bytes)))
        assert (ct[words:] == 0xA5A5A5A5).all(), "FSE_buildCTable wrote past FSE_CTABLE_SIZE_U32(tableLog, maxSymbolValue)"
        return r, ct[:words]

    def fse_build_dtable(self, norm, max_sv, table_log):
        norm = np.ascontiguousarray(norm, dtype=np.int16)
        words = 1 + (1 << max(min(table_log, 12), 0))
        dt = np.zeros(words + 4, dtype=np.uint32)
        dt[words:] = 0xA5A5A5A5
        self.lib.FSEHIP_FSE_buildDTable.restype = SZ
        r = int(self.lib.FSEHIP_FSE_buildDTable(dt.ctypes.data_as(VP), norm.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(table_log)))
        assert (dt[words:] == 0xA5A5A5A5).all(), "FSE_buildDTable wrote past FSE_DTABLE_SIZE_U32(tableLog)"
        return r, dt[:words]

    def fse_compress2(self, src, max_sv=255, table_log=11, cap=None):
        return self._single("FSEHIP_FSE_compress2", fse_compress_bound(len(src)) if cap is None else cap, src, C.c_uint(max_sv), C.c_uint(table_log))

    def fse_decompress(self, csrc, cap):
        return self._single("FSEHIP_FSE_decompress", cap, csrc)


# ---------------------------------------------------------------------------------------------------------
#  Huff0 (lib/huf.h)
# ---------------------------------------------------------------------------------------------------------
def _huf_methods():
    def huf_workspace(self, n_blocks, decompress=False, device="cuda"):
        fn = self.lib.FSEHIP_HUF_decompress_batch_workspaceSize if decompress else self.lib.FSEHIP_HUF_compress_batch_workspaceSize
        return torch.empty(int(fn(SZ(n_blocks))), dtype=torch.uint8, device=device)

    def huf_compress_batch(self, src, table_log=11, max_symbol_value=255, sizes=None, dst=None, dst_capacity=None, results=None, workspace=None):
        n = _blocks(src, "src").shape[0]
        cap = huf_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=src.device)
        if workspace is None:
            workspace = self.huf_workspace(n, False, src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_HUF_compress_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(results), _ptr(src), SZ(src.stride(0)), ps, uni,
                                                  C.c_uint(max_symbol_value), C.c_uint(table_log), SZ(n), _ptr(workspace),
                                                  SZ(workspace.numel()), _stream()), "HUF_compress_batch")
        if g:
            g.check("HUF_compress_batch")
        return dst, results

    def huf_decompress_batch(self, csrc, csizes, dst_sizes, dst=None, results=None, workspace=None):
        n = _blocks(csrc, "csrc").shape[0]
        width = int(dst_sizes) if isinstance(dst_sizes, numbers.Integral) else int(dst_sizes.max().item())
        g = None
        if dst is None:
            dst, g = self._dst(n, width, csrc.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=csrc.device)
        if workspace is None:
            workspace = self.huf_workspace(n, True, csrc.device)
        pc, unic, keepc = _sizes_arg(csizes, csrc)
        pd, unid, keepd = _sizes_arg(dst_sizes, csrc)
        _check(self.lib.FSEHIP_HUF_decompress_batch(_ptr(dst), SZ(dst.stride(0)), pd, unid, _ptr(results), _ptr(csrc), SZ(csrc.stride(0)), pc, unic,
                                                    SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()), "HUF_decompress_batch")
        if g:
            g.check("HUF_decompress_batch", dst_sizes)
        return dst, results

    def huf_compress4x_using_ctable_batch(self, src, ctables, sizes=None, dst_capacity=None, shared_table=False, dst=None, results=None):
        """ctables: (n, 256) int32/uint32 HUF_CElt entries (val | nbBits << 16)"""
        n = _blocks(src, "src").shape[0]
        cap = huf_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=src.device) if results is None else results
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        stride = 0 if shared_table else ctables.stride(0)
        _check(self.lib.FSEHIP_HUF_compress4X_usingCTable_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(res), _ptr(src), SZ(src.stride(0)),
                                                                ps, uni, _ptr(ctables), SZ(stride), SZ(n), _stream()),
               "HUF_compress4X_usingCTable_batch")
        if g:
            g.check("HUF_compress4X_usingCTable_batch")
        return dst, res

    def huf_compress1x_using_ctable_batch(self, src, ctables, sizes=None, dst_capacity=None, shared_table=False, dst=None, results=None):
        """HUF_compress1X_usingCTable over a batch (lib/huf.h:290): one stream per block"""
        n = _blocks(src, "src").shape[0]
        cap = huf_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=src.device) if results is None else results
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        stride = 0 if shared_table else ctables.stride(0)
        _check(self.lib.FSEHIP_HUF_compress1X_usingCTable_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(res), _ptr(src), SZ(src.stride(0)),
                                                                ps, uni, _ptr(ctables), SZ(stride), SZ(n), _stream()),
               "HUF_compress1X_usingCTable_batch")
        if g:
            g.check("HUF_compress1X_usingCTable_batch")
        return dst, res

    def huf_decompress4x_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None):
        """HUF_decompress4X_usingDTable over a batch: X1 (tableType 0) and X2 (tableType 1) tables, chosen per block"""
        return self.huf_decompress4x1_using_dtable_batch(csrc, csizes, dtables, dst_sizes, max_table_log, shared_table, dst=dst, results=results,
                                                         _fn="FSEHIP_HUF_decompress4X_usingDTable_batch")

    def huf_decompress4x1_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None,
                                             _fn="FSEHIP_HUF_decompress4X1_usingDTable_batch"):
        n = _blocks(csrc, "csrc").shape[0]
        g = None
        if dst is None:
            width = int(dst_sizes) if isinstance(dst_sizes, numbers.Integral) else int(dst_sizes.max().item())
            dst, g = self._dst(n, width, csrc.device, zero=not self.guard)
        res = torch.zeros(n, dtype=torch.int64, device=csrc.device) if results is None else results
        pc, unic, keepc = _sizes_arg(csizes, csrc)
        pd, unid, keepd = _sizes_arg(dst_sizes, csrc)
        stride = 0 if shared_table else dtables.stride(0)
        _check(getattr(self.lib, _fn)(_ptr(dst), SZ(dst.stride(0)), pd, unid, _ptr(res), _ptr(csrc), SZ(csrc.stride(0)),
                                      pc, unic, _ptr(dtables), SZ(stride), C.c_uint(max_table_log), SZ(n), _stream()), _fn)
        if g:
            g.check(_fn, dst_sizes)
        return dst, res

    def huf_build_ctable_batch(self, src, table_log=11, max_symbol_value=255, sizes=None, header_capacity=256):
        """HUF_buildCTable_batch: (ctables (n, 256) int32 HUF_CElt, headers (n, header_capacity) uint8, results)"""
        n = _blocks(src, "src").shape[0]
        ct = torch.zeros((n, 256), dtype=torch.int32, device=src.device)
        hdr, g = self._dst(n, header_capacity, src.device, zero=True)
        res = torch.zeros(n, dtype=torch.int64, device=src.device)
        ws = torch.empty(int(self.lib.FSEHIP_HUF_buildCTable_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_HUF_buildCTable_batch(_ptr(ct), SZ(ct.stride(0)), _ptr(hdr), SZ(hdr.stride(0)), SZ(header_capacity), _ptr(res), _ptr(src),
                                                     SZ(src.stride(0)), ps, uni, C.c_uint(max_symbol_value), C.c_uint(table_log), SZ(n), _ptr(ws),
                                                     SZ(ws.numel()), _stream()), "HUF_buildCTable_batch")
        if g:
            g.check("HUF_buildCTable_batch")
        return ct, hdr, res

    # the Huff0 table glue on the caller's statistics (include/fsehip.h "Table glue, step by step"; lib/huf.h:204-218)
    def huf_build_ctable_from_count_batch(self, counts, max_symbol_values, max_nb_bits=0, ctables=None, ctable_stride_u32=256, results=None):
        """HUF_buildCTable per row of `counts` (n, 256) int32: (ctables (n, ctable_stride_u32) int32 HUF_CElt -- zero above each row's
        maxSymbolValue --, results = table log or error).  Entries of a row above its maxSymbolValue are ignored."""
        n = counts.shape[0]
        if ctables is None:
            ctables = torch.zeros((n, ctable_stride_u32), dtype=torch.int32, device=counts.device)
        res = torch.zeros(n, dtype=torch.int64, device=counts.device) if results is None else results
        _check(self.lib.FSEHIP_HUF_buildCTable_fromCount_batch(_ptr(ctables), SZ(ctables.stride(0)), _ptr(counts), SZ(counts.stride(0)), _ptr(max_symbol_values),
                                                               C.c_uint(max_nb_bits), SZ(n), _ptr(res), _stream()), "HUF_buildCTable_fromCount_batch")
        return ctables, res

    def huf_write_ctable_batch(self, ctables, max_symbol_values, huff_log, header_capacity=256, header_stride=None, results=None):
        """HUF_writeCTable per row of `ctables` (n, >= 256) int32 HUF_CElt: (headers (n, header_stride or header_capacity) uint8 pre-filled with
        0xA5, results = header bytes or error).  Entries of a row above its maxSymbolValue are ignored."""
        n = ctables.shape[0]
        hdr, g = self._dst(n, max(header_stride or 0, header_capacity), ctables.device)
        hdr.fill_(0xA5)
        res = torch.zeros(n, dtype=torch.int64, device=ctables.device) if results is None else results
        _check(self.lib.FSEHIP_HUF_writeCTable_batch(_ptr(hdr), SZ(hdr.stride(0)), SZ(header_capacity), _ptr(ctables), SZ(ctables.stride(0)), _ptr(max_symbol_values),
                                                     C.c_uint(huff_log), SZ(n), _ptr(res), _stream()), "HUF_writeCTable_batch")
        if g:                                                  # the guard bytes behind the row, and what lies between the capacity and the row's end
            g.check("HUF_writeCTable_batch")
            if bool((hdr[:, header_capacity:] != 0xA5).any().item()):
                raise AssertionError("HUF_writeCTable_batch wrote past its header capacity (%d) inside the row" % header_capacity)
        return hdr, res

    def huf_read_dtable_x1_batch(self, csrc, csizes, max_table_log=11):
        """HUF_readDTableX1_batch: (dtables (n, 1 + (1 << max_table_log)) int32, results = header bytes or error)"""
        n = _blocks(csrc, "csrc").shape[0]
        dt = torch.zeros((n, 1 + (1 << max_table_log)), dtype=torch.int32, device=csrc.device)
        res = torch.zeros(n, dtype=torch.int64, device=csrc.device)
        ws = torch.empty(int(self.lib.FSEHIP_HUF_readDTableX1_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=csrc.device)
        ps, uni, keep = _sizes_arg(csizes, csrc)
        _check(self.lib.FSEHIP_HUF_readDTableX1_batch(_ptr(dt), SZ(dt.stride(0)), C.c_uint(max_table_log), _ptr(res), _ptr(csrc), SZ(csrc.stride(0)), ps, uni,
                                                      SZ(n), _ptr(ws), SZ(ws.numel()), _stream()), "HUF_readDTableX1_batch")
        return dt, res

    def huf_read_dtable_x2_batch(self, csrc, csizes, max_table_log=12, dtables=None, results=None, workspace=None):
        """HUF_readDTableX2_batch: (dtables (n, 1 + (1 << max_table_log)) int32 -- double-symbol cells --, results = header bytes or error).
        max_table_log is DTableDesc.maxTableLog as the reference reads it (above 12: every block fails, nothing is written)"""
        n = _blocks(csrc, "csrc").shape[0]
        g = None
        if dtables is None:
            dtables, g = self._dst(n, 1 + (1 << min(max_table_log, 12)), csrc.device, zero=True, dtype=torch.int32)
        res = torch.zeros(n, dtype=torch.int64, device=csrc.device) if results is None else results
        if workspace is None:
            workspace = torch.empty(int(self.lib.FSEHIP_HUF_readDTableX2_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=csrc.device)
        ps, uni, keep = _sizes_arg(csizes, csrc)
        _check(self.lib.FSEHIP_HUF_readDTableX2_batch(_ptr(dtables), SZ(dtables.stride(0)), C.c_uint(max_table_log), _ptr(res), _ptr(csrc), SZ(csrc.stride(0)),
                                                      ps, uni, SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()), "HUF_readDTableX2_batch")
        if g:
            g.check("HUF_readDTableX2_batch")
        return dtables, res

    def huf_decompress4x2_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None):
        """HUF_decompress4X2_usingDTable over a batch: double-symbol tables only (a tableType 0 table: GENERIC)"""
        return self.huf_decompress4x1_using_dtable_batch(csrc, csizes, dtables, dst_sizes, max_table_log, shared_table, dst=dst, results=results,
                                                         _fn="FSEHIP_HUF_decompress4X2_usingDTable_batch")

    def huf_decompress1x2_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None):
        """HUF_decompress1X2_usingDTable over a batch: one stream per block, double-symbol tables only"""
        return self.huf_decompress4x1_using_dtable_batch(csrc, csizes, dtables, dst_sizes, max_table_log, shared_table, dst=dst, results=results,
                                                         _fn="FSEHIP_HUF_decompress1X2_usingDTable_batch")

    def huf_decompress_packed_batch(self, packed, offsets, dst_sizes, dst=None, results=None, workspace=None):
        n = offsets.numel() - 1
        width = int(dst_sizes) if isinstance(dst_sizes, numbers.Integral) else int(dst_sizes.max().item())
        g = None
        if dst is None:
            dst, g = self._dst(n, width, packed.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=packed.device)
        if workspace is None:
            workspace = self.huf_workspace(n, True, packed.device)
        pd, unid, keepd = _sizes_arg(dst_sizes, packed)
        _check(self.lib.FSEHIP_HUF_decompress_packed_batch(_ptr(dst), SZ(dst.stride(0)), pd, unid, _ptr(results), _ptr(packed), _ptr(offsets), SZ(n),
                                                           _ptr(workspace), SZ(workspace.numel()), _stream()), "HUF_decompress_packed_batch")
        if g:
            g.check("HUF_decompress_packed_batch", dst_sizes)
        return dst, results

    def huf_decompress1x1_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None):
        """HUF_decompress1X1_usingDTable over a batch: one stream per block"""
        return self.huf_decompress4x1_using_dtable_batch(csrc, csizes, dtables, dst_sizes, max_table_log, shared_table, dst=dst, results=results,
                                                         _fn="FSEHIP_HUF_decompress1X1_usingDTable_batch")

    def huf_decompress1x_using_dtable_batch(self, csrc, csizes, dtables, dst_sizes, max_table_log=12, shared_table=False, dst=None, results=None):
        return self.huf_decompress4x1_using_dtable_batch(csrc, csizes, dtables, dst_sizes, max_table_log, shared_table, dst=dst, results=results,
                                                         _fn="FSEHIP_HUF_decompress1X_usingDTable_batch")

    def huf_decompress1x1_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_decompress1X1_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    def huf_decompress1x_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_decompress1X_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    # the Huff0 advanced flow on host pointers (lib/huf.h:141-167,204-218,288,299-304): same argument order as the reference, numpy in / out
    def huf_build_ctable(self, count, max_sv, max_nb_bits=0):
        """HUF_buildCTable: (table log or error, HUF_CElt[256] as uint32 -- entries beyond max_sv stay zero)"""
        count = np.ascontiguousarray(count, dtype=np.uint32)
        celt = np.zeros(256, dtype=np.uint32)
        self.lib.FSEHIP_HUF_buildCTable.restype = SZ
        return int(self.lib.FSEHIP_HUF_buildCTable(celt.ctypes.data_as(VP), count.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(max_nb_bits))), celt

    def huf_write_ctable(self, celt, max_sv, huff_log, cap=256):
        celt = np.ascontiguousarray(celt, dtype=np.uint32)
        out = np.full(max(cap, 1) + 8, 0xA5, dtype=np.uint8)
        self.lib.FSEHIP_HUF_writeCTable.restype = SZ
        r = int(self.lib.FSEHIP_HUF_writeCTable(out.ctypes.data_as(VP), SZ(cap), celt.ctypes.data_as(VP), C.c_uint(max_sv), C.c_uint(huff_log)))
        assert (out[cap:] == 0xA5).all(), "HUF_writeCTable wrote past maxDstSize"
        return r, out[:cap]

    def huf_read_dtable_x1(self, src, max_table_log=12):
        """HUF_readDTableX1 into a DTable made by HUF_CREATE_STATIC_DTABLEX1(DTable, max_table_log): (header size or error, DTable)"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        dt = np.zeros(1 + (1 << 11), dtype=np.uint32)
        dt[0] = (max_table_log - 1) * 0x01000001
        self.lib.FSEHIP_HUF_readDTableX1.restype = SZ
        return int(self.lib.FSEHIP_HUF_readDTableX1(dt.ctypes.data_as(VP), src.ctypes.data_as(VP), SZ(src.size))), dt

    def huf_read_dtable_x2(self, src, max_table_log=12, wksp_bytes=None, dtable=None):
        """HUF_readDTableX2 (wksp_bytes None) / HUF_readDTableX2_wksp into a DTable made by HUF_CREATE_STATIC_DTABLEX2(DTable, max_table_log), or into
        `dtable` (uint32, written in place): (header size or error, DTable)"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if dtable is None:
            dtable = np.zeros(1 + (1 << 12), dtype=np.uint32)
            dtable[0] = max_table_log * 0x01000001
        if wksp_bytes is None:
            self.lib.FSEHIP_HUF_readDTableX2.restype = SZ
            return int(self.lib.FSEHIP_HUF_readDTableX2(dtable.ctypes.data_as(VP), src.ctypes.data_as(VP), SZ(src.size))), dtable
        ws = np.zeros(max(wksp_bytes, 4) // 4 + 1, dtype=np.uint32)
        self.lib.FSEHIP_HUF_readDTableX2_wksp.restype = SZ
        return int(self.lib.FSEHIP_HUF_readDTableX2_wksp(dtable.ctypes.data_as(VP), src.ctypes.data_as(VP), SZ(src.size), ws.ctypes.data_as(VP), SZ(wksp_bytes))), dtable

    def _huf_x2(self, base, csrc, dst_size, dctx, wksp_bytes):
        if dctx is None:
            fname, extra = base, ()
        elif wksp_bytes is None:
            fname, extra = base + "_DCtx", ()
        else:
            self._x2_ws = np.zeros(max(wksp_bytes, 4) // 4 + 1, dtype=np.uint32)
            fname, extra = base + "_DCtx_wksp", (self._x2_ws.ctypes.data_as(VP), SZ(wksp_bytes))
        getattr(self.lib, fname).restype = SZ
        if dctx is None:
            return self._single(fname, dst_size, csrc)
        csrc = np.ascontiguousarray(csrc, dtype=np.uint8)
        out = np.zeros(max(dst_size, 1) + 16, dtype=np.uint8)
        out[dst_size:] = 0xA5
        r = int(getattr(self.lib, fname)(dctx.ctypes.data_as(VP), out.ctypes.data_as(VP), SZ(dst_size), csrc.ctypes.data_as(VP), SZ(csrc.size), *extra))
        assert (out[dst_size:] == 0xA5).all(), "%s wrote past dstSize" % fname
        return r, out[:dst_size]

    def huf_decompress4x2(self, csrc, dst_size, dctx=None, wksp_bytes=None):
        """HUF_decompress4X2 / HUF_decompress4X2_DCtx (dctx: uint32 DTable, receives the table) / HUF_decompress4X2_DCtx_wksp (wksp_bytes too)"""
        return self._huf_x2("FSEHIP_HUF_decompress4X2", csrc, dst_size, dctx, wksp_bytes)

    def huf_decompress1x2(self, csrc, dst_size, dctx=None, wksp_bytes=None):
        """HUF_decompress1X2 / HUF_decompress1X2_DCtx / HUF_decompress1X2_DCtx_wksp: one stream per block"""
        return self._huf_x2("FSEHIP_HUF_decompress1X2", csrc, dst_size, dctx, wksp_bytes)

    def huf_decompress4x2_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        self.lib.FSEHIP_HUF_decompress4X2_usingDTable.restype = SZ
        return self._single("FSEHIP_HUF_decompress4X2_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    def huf_decompress1x2_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        self.lib.FSEHIP_HUF_decompress1X2_usingDTable.restype = SZ
        return self._single("FSEHIP_HUF_decompress1X2_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    def huf_compress1x(self, src, max_sv=255, huff_log=11, cap=None):
        return self._single("FSEHIP_HUF_compress1X", huf_compress_bound(len(src)) if cap is None else cap, src, C.c_uint(max_sv), C.c_uint(huff_log))

    def huf_decompress4x1(self, csrc, dst_size):
        self.lib.FSEHIP_HUF_decompress4X1.restype = SZ
        return self._single("FSEHIP_HUF_decompress4X1", dst_size, csrc)

    def huf_decompress1x1(self, csrc, dst_size):
        self.lib.FSEHIP_HUF_decompress1X1.restype = SZ
        return self._single("FSEHIP_HUF_decompress1X1", dst_size, csrc)

    # layer 1
    def huf_compress2(self, src, max_sv=255, huff_log=11, cap=None):
        return self._single("FSEHIP_HUF_compress2", huf_compress_bound(len(src)) if cap is None else cap, src, C.c_uint(max_sv), C.c_uint(huff_log))

    def huf_decompress(self, csrc, dst_size):
        return self._single("FSEHIP_HUF_decompress", dst_size, csrc)

    def huf_compress1x_using_ctable(self, src, celt, cap=None):
        celt = np.ascontiguousarray(celt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_compress1X_usingCTable", huf_compress_bound(len(src)) if cap is None else cap, src, celt.ctypes.data_as(VP))

    def huf_compress4x_using_ctable(self, src, celt, cap=None):
        celt = np.ascontiguousarray(celt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_compress4X_usingCTable", huf_compress_bound(len(src)) if cap is None else cap, src, celt.ctypes.data_as(VP))

    def huf_decompress4x1_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_decompress4X1_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    def huf_decompress4x_using_dtable(self, csrc, dt, dst_size):
        dt = np.ascontiguousarray(dt, dtype=np.uint32)
        return self._single("FSEHIP_HUF_decompress4X_usingDTable", dst_size, csrc, dt.ctypes.data_as(VP))

    for f in (huf_decompress1x1_using_dtable_batch, huf_decompress1x_using_dtable_batch, huf_decompress1x1_using_dtable, huf_decompress1x_using_dtable,
              huf_decompress_packed_batch, huf_build_ctable_batch, huf_build_ctable_from_count_batch, huf_write_ctable_batch, huf_read_dtable_x1_batch, huf_workspace, huf_compress_batch, huf_decompress_batch, huf_compress4x_using_ctable_batch, huf_compress1x_using_ctable_batch,
              huf_decompress4x1_using_dtable_batch, huf_decompress4x_using_dtable_batch, huf_compress2, huf_decompress, huf_compress1x_using_ctable,
              huf_compress4x_using_ctable, huf_decompress4x1_using_dtable, huf_decompress4x_using_dtable,
              huf_build_ctable, huf_write_ctable, huf_read_dtable_x1, huf_compress1x, huf_decompress4x1, huf_decompress1x1,
              huf_read_dtable_x2_batch, huf_decompress4x2_using_dtable_batch, huf_decompress1x2_using_dtable_batch, huf_read_dtable_x2, _huf_x2,
              huf_decompress4x2, huf_decompress1x2, huf_decompress4x2_using_dtable, huf_decompress1x2_using_dtable):
        setattr(FseHip, f.__name__, f)


_huf_methods()


def _frame_methods():
    # .fse frames on host buffers (programs/fileio.c): FSEHIP_frame_compress / FSEHIP_frame_decompress
    def frame_compress(self, src, block_size_id=5, codec=0, cap=None):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        self.lib.FSEHIP_frame_compressBound.restype = C.c_size_t
        bound = int(self.lib.FSEHIP_frame_compressBound(SZ(src.size), C.c_uint(block_size_id)))
        if cap is None:
            cap = bound if bound < (1 << 62) else 16
        return self._single("FSEHIP_frame_compress", cap, src, C.c_uint(block_size_id), C.c_int(codec))

    def frame_decompress(self, frame, cap):
        return self._single("FSEHIP_frame_decompress", cap, frame)

    def _frames(self, fname, srcs, caps, n_threads, *extra):
        # many frames per call: arrays of host pointers / sizes; every destination carries a 0xA5 tail like _single's
        srcs = [np.ascontiguousarray(x, dtype=np.uint8) for x in srcs]
        n = len(srcs)
        outs = [np.zeros(max(c, 1) + 16, dtype=np.uint8) for c in caps]
        for o, c in zip(outs, caps):
            o[c:] = 0xA5
        PA, SA = C.c_void_p * max(n, 1), C.c_size_t * max(n, 1)
        dsts = PA(*[o.ctypes.data for o in outs]); dcap = SA(*caps)
        sp = PA(*[x.ctypes.data for x in srcs]); ssz = SA(*[x.size for x in srcs])
        res = SA()
        fn = getattr(self.lib, fname)
        fn.restype = C.c_size_t
        r = int(fn(dsts, dcap, sp, ssz, res, SZ(n), *extra, C.c_uint(n_threads)))
        assert r == 0, "%s: %#x" % (fname, r)
        for o, c in zip(outs, caps):
            assert (o[c:] == 0xA5).all(), "%s wrote past dstCapacity" % fname
        return [(int(res[i]), outs[i][:caps[i]]) for i in range(n)]

    def frame_compress_batch(self, srcs, block_size_id=5, codec=0, caps=None, n_threads=0):
        self.lib.FSEHIP_frame_compressBound.restype = C.c_size_t
        if caps is None:
            caps = [int(self.lib.FSEHIP_frame_compressBound(SZ(np.asarray(x).size), C.c_uint(block_size_id))) for x in srcs]
            caps = [c if c < (1 << 62) else 16 for c in caps]
        return self._frames("FSEHIP_frame_compress_batch", srcs, caps, n_threads, C.c_uint(block_size_id), C.c_int(codec))

    def frame_decompress_batch(self, frames, caps, n_threads=0):
        return self._frames("FSEHIP_frame_decompress_batch", frames, caps, n_threads)

    for f in (_frames, frame_compress_batch, frame_decompress_batch, frame_compress, frame_decompress):
        setattr(FseHip, f.__name__, f)


_frame_methods()


class FrameInfo(C.Structure):
    """FSEHIP_FrameInfo (include/fsehip.h): what a frame says about itself without a block being decoded"""
    _fields_ = [("contentBound", C.c_uint64), ("nBlocks", C.c_uint64), ("status", C.c_uint32), ("checksum22", C.c_uint32),
                ("codec", C.c_uint8), ("blockSizeId", C.c_uint8), ("reserved", C.c_uint8 * 6)]


FRAME_INFO_DTYPE = np.dtype([("contentBound", "<u8"), ("nBlocks", "<u8"), ("status", "<u4"), ("checksum22", "<u4"),
                             ("codec", "u1"), ("blockSizeId", "u1"), ("reserved", "u1", (6,))])


def _frame_dev_methods():
    # .fse frames on DEVICE buffers (csrc/frame_dev.hip): many contents <-> many frames in one flat CUDA uint8 tensor each, cut by offsets
    # (n + 1 entries).  Offsets come as a host sequence / numpy array (uploaded here) or as a CUDA int64 tensor (used as it is: with
    # max_total_blocks, dst, results and workspace given too, the call is launches only and can be captured into a graph).
    def _offsets(self, offsets, device, need_host):
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
            dev = offsets.to(torch.int64).contiguous()
            return dev, (dev.cpu().numpy().astype(np.uint64) if need_host else None)
        host = np.ascontiguousarray(np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets), dtype=np.uint64)
        if host.ndim != 1 or host.size < 1:
            raise ValueError("offsets: one entry more than items")
        return torch.from_numpy(host.astype(np.int64)).to(device), host

    def _flat(t, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError("%s must be a contiguous 1-D CUDA uint8 tensor" % what)
        return t

    def frame_block_count(self, n, block_size_id=5):
        self.lib.FSEHIP_frame_blockCount.restype = SZ
        return int(self.lib.FSEHIP_frame_blockCount(SZ(int(n)), C.c_uint(block_size_id)))

    def frame_dbatch_plan(self, sizes, block_size_id=5):
        """destination offsets of frame_compress_dbatch for contents of these sizes: every frame gets exactly FSEHIP_frame_compressBound bytes"""
        self.lib.FSEHIP_frame_compressBound.restype = SZ
        bounds = [int(self.lib.FSEHIP_frame_compressBound(SZ(int(n)), C.c_uint(block_size_id))) for n in sizes]
        if any(b >= (1 << 62) for b in bounds):
            raise ValueError("block_size_id %r" % (block_size_id,))
        return np.concatenate([[0], np.cumsum(np.asarray(bounds, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)

    def frame_dbatch_workspace(self, n_frames, max_total_blocks, block_size_id=None, codec=0, device="cuda"):
        """block_size_id None: the reader's workspace"""
        if block_size_id is None:
            self.lib.FSEHIP_frame_decompress_dbatch_workspaceSize.restype = SZ
            n = int(self.lib.FSEHIP_frame_decompress_dbatch_workspaceSize(SZ(n_frames), SZ(max_total_blocks)))
        else:
            self.lib.FSEHIP_frame_compress_dbatch_workspaceSize.restype = SZ
            n = int(self.lib.FSEHIP_frame_compress_dbatch_workspaceSize(SZ(n_frames), SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(codec)))
            if n >= (1 << 62):
                raise ValueError("block_size_id %r / codec %r" % (block_size_id, codec))
        return torch.empty(max(n, 1), dtype=torch.uint8, device=device)

    def xxh32_batch(self, data, offsets, seed=0):
        """hashes[i] = XXH32(data[offsets[i]:offsets[i+1]], seed), as an int64 tensor of values below 2**32"""
        _flat(data, "data")
        off, _ = self._offsets(offsets, data.device, False)
        n = off.numel() - 1
        h = torch.zeros(max(n, 1), dtype=torch.int32, device=data.device)
        _check(self.lib.FSEHIP_XXH32_batch(_ptr(h), _ptr(data), _ptr(off), SZ(n), C.c_uint32(seed & 0xFFFFFFFF), _stream()), "XXH32_batch")
        return h[:n].to(torch.int64) & 0xFFFFFFFF

    def frame_compress_dbatch(self, src, src_offsets, block_size_id=5, codec=0, dst=None, dst_offsets=None, max_total_blocks=None, workspace=None, results=None):
        """-> (frames, dst_offsets, results): frame i = frames[dst_offsets[i] : dst_offsets[i] + results[i]]; a negative result -c is error code c"""
        _flat(src, "src")
        need_host = dst_offsets is None or max_total_blocks is None
        soff, shost = self._offsets(src_offsets, src.device, need_host)
        n = soff.numel() - 1
        if dst_offsets is None:
            dst_offsets = self.frame_dbatch_plan(np.diff(shost), block_size_id)
        doff, dhost = self._offsets(dst_offsets, src.device, dst is None)
        if doff.numel() != n + 1:
            raise ValueError("dst_offsets: one entry per frame and one more")
        if max_total_blocks is None:
            max_total_blocks = sum(self.frame_block_count(int(x), block_size_id) for x in np.diff(shost)) if block_size_id <= 6 else 0
        g = None
        if dst is None:
            total = int(dhost[-1])
            dst, g = self._dst(1, total, src.device)
            dst = dst[0]
        res = torch.zeros(max(n, 1), dtype=torch.int64, device=src.device)[:n] if results is None else results
        ws = workspace if workspace is not None else self.frame_dbatch_workspace(n, max_total_blocks, min(block_size_id, 6), codec if codec in (0, 1) else 0, src.device)
        _check(self.lib.FSEHIP_frame_compress_dbatch(_ptr(dst), _ptr(doff), _ptr(res), _ptr(src), _ptr(soff), SZ(n), SZ(max_total_blocks),
                                                     C.c_uint(block_size_id), C.c_int(codec), _ptr(ws), SZ(ws.numel()), _stream()), "frame_compress_dbatch")
        if g is not None:
            g.check("frame_compress_dbatch")
            # ... and inside the slots: the writer's contract is the frame's bytes and nothing else (include/fsehip.h)
            total = int(dhost[-1])
            if total:
                idx = torch.arange(total, device=src.device)
                slot = torch.searchsorted(doff[1:].contiguous(), idx, right=True).clamp(max=n - 1)
                beyond = (idx - doff[slot]) >= res[slot].clamp(min=0)
                assert bool((g.full[0, :total][beyond] == g.fill).all()), "frame_compress_dbatch wrote behind a frame's last byte"
        return dst, doff, res

    def frame_decompress_dbatch(self, frames, frame_offsets, dst_offsets, dst=None, max_total_blocks=None, workspace=None, results=None):
        """-> (dst, results): content i = dst[dst_offsets[i] : dst_offsets[i] + results[i]]; capacity of slot i = dst_offsets[i+1] - dst_offsets[i]"""
        _flat(frames, "frames")
        foff, fhost = self._offsets(frame_offsets, frames.device, max_total_blocks is None)
        n = foff.numel() - 1
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None)
        if doff.numel() != n + 1:
            raise ValueError("dst_offsets: one entry per frame and one more")
        if max_total_blocks is None:                      # a frame of F bytes: at most (F - 8) / 2 blocks
            max_total_blocks = int(sum(max(int(x) - 8, 0) // 2 for x in np.diff(fhost)))
        g = None
        if dst is None:
            dst, g = self._dst(1, int(dhost[-1]), frames.device)
            dst = dst[0]
        res = torch.zeros(max(n, 1), dtype=torch.int64, device=frames.device)[:n] if results is None else results
        ws = workspace if workspace is not None else self.frame_dbatch_workspace(n, max_total_blocks, None, 0, frames.device)
        _check(self.lib.FSEHIP_frame_decompress_dbatch(_ptr(dst), _ptr(doff), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), SZ(max_total_blocks),
                                                       _ptr(ws), SZ(ws.numel()), _stream()), "frame_decompress_dbatch")
        if g is not None:
            g.check("frame_decompress_dbatch")
        return dst, res

    # ---- frames of unknown size (fsehip.h, FSEHIP_FrameInfo): what a frame announces, the plan made from it, and the reader behind the plan
    def _align_log(align_log):
        if not isinstance(align_log, numbers.Integral) or not 0 <= align_log <= 12:
            raise ValueError("align_log %r: slots are aligned to 1 << 0 .. 1 << 12 bytes" % (align_log,))
        return int(align_log)

    def frame_inspect(self, frame):
        """-> (result, info): result = the content bound (a capacity, not a size) or, >= 2**64 - 8, an error code; info = the FSEHIP_FrameInfo
        fields as a dict.  Host arithmetic: needs no device."""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        fi = FrameInfo()
        self.lib.FSEHIP_frame_inspect.restype = SZ
        r = int(self.lib.FSEHIP_frame_inspect(C.byref(fi), frame.ctypes.data_as(VP), SZ(frame.size)))
        return r, dict(content_bound=int(fi.contentBound), n_blocks=int(fi.nBlocks), status=int(fi.status), checksum22=int(fi.checksum22),
                       codec=int(fi.codec), block_size_id=int(fi.blockSizeId), reserved=bytes(fi.reserved))

    def frame_plan_dbatch(self, frames, frame_offsets, capacity=None, align_log=0, with_infos=False, dst_offsets=None, block_first=None, workspace=None):
        """-> (dst_offsets, block_first[, infos]): int64 CUDA tensors of n + 1 entries -- dst_offsets[i] = min(U[i], capacity) with U the running
        sum of the frames' content bounds rounded up to 1 << align_log, block_first[i] = the blocks of the frames before i; infos: an (n, 32)
        uint8 tensor, `infos.cpu().numpy().view(FRAME_INFO_DTYPE)[:, 0]` names its fields.  capacity None: the sizing query (dst_offsets[n] =
        the capacity all frames need, block_first[n] = the exact max_total_blocks).  Launches only."""
        align_log = _align_log(align_log)
        _flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        n = foff.numel() - 1
        doff = torch.empty(n + 1, dtype=torch.int64, device=frames.device) if dst_offsets is None else dst_offsets
        bfirst = torch.empty(n + 1, dtype=torch.int64, device=frames.device) if block_first is None else block_first
        infos = torch.empty((max(n, 1), C.sizeof(FrameInfo)), dtype=torch.uint8, device=frames.device)[:n] if with_infos else None
        if workspace is None:
            self.lib.FSEHIP_frame_plan_dbatch_workspaceSize.restype = SZ
            workspace = torch.empty(max(int(self.lib.FSEHIP_frame_plan_dbatch_workspaceSize(SZ(n))), 1), dtype=torch.uint8, device=frames.device)
        cap = (1 << 64) - 1 if capacity is None else int(capacity)
        _check(self.lib.FSEHIP_frame_plan_dbatch(_ptr(doff), _ptr(bfirst), _ptr(infos), _ptr(frames), _ptr(foff), SZ(n), C.c_uint64(cap), C.c_uint(align_log),
                                                 _ptr(workspace), SZ(workspace.numel()), _stream()), "frame_plan_dbatch")
        return (doff, bfirst, infos) if with_infos else (doff, bfirst)

    def frame_decompress_packed_dbatch(self, frames, frame_offsets, dst=None, capacity=None, max_total_blocks=None, align_log=0, dst_offsets=None,
                                       workspace=None, results=None):
        """-> (dst, dst_offsets, results): content i = dst[dst_offsets[i] : dst_offsets[i] + results[i]], its slot what frame_plan_dbatch gives it
        for `capacity` (default: dst's size).  dst None: a sizing query first, whose two totals are read back -- the destination (guarded in guard
        mode) holds every frame's bound and the block promise is exact.  With dst, max_total_blocks, dst_offsets, workspace and results given the
        call is launches only and can be captured into a graph."""
        align_log = _align_log(align_log)
        _flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        n = foff.numel() - 1
        if dst is None or max_total_blocks is None:
            doff, bfirst = self.frame_plan_dbatch(frames, foff, None, align_log)
            need, blocks = (int(x) for x in torch.stack([doff[n], bfirst[n]]).cpu())
            if max_total_blocks is None:
                max_total_blocks = blocks
        g = None
        if dst is None:
            capacity = need if capacity is None else int(capacity)
            dst, g = self._dst(1, capacity, frames.device)
            dst = dst[0]
        else:
            _flat(dst, "dst")
            capacity = dst.numel() if capacity is None else int(capacity)
            if capacity > dst.numel():
                raise ValueError("capacity %d: dst holds %d bytes" % (capacity, dst.numel()))
        doff = torch.empty(n + 1, dtype=torch.int64, device=frames.device) if dst_offsets is None else dst_offsets
        res = torch.zeros(max(n, 1), dtype=torch.int64, device=frames.device)[:n] if results is None else results
        if workspace is None:
            self.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = SZ
            workspace = torch.empty(max(int(self.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(n), SZ(max_total_blocks))), 1),
                                    dtype=torch.uint8, device=frames.device)
        _check(self.lib.FSEHIP_frame_decompress_packed_dbatch(_ptr(dst), SZ(capacity), _ptr(doff), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), SZ(max_total_blocks),
                                                              C.c_uint(align_log), _ptr(workspace), SZ(workspace.numel()), _stream()), "frame_decompress_packed_dbatch")
        if g is not None:
            g.check("frame_decompress_packed_dbatch")
        return dst, doff, res

    # ---- the packed writer (fsehip.h, FSEHIP_frame_compress_packed_dbatch): frames back to back at their real sizes, offsets from the device
    def frame_packed_bound(self, total_src_bytes, n_frames, total_blocks, align_log=0):
        """a capacity of frame_compress_packed_dbatch at which no frame fails for lack of room.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_frame_packedBound.restype = SZ
        r = int(self.lib.FSEHIP_frame_packedBound(SZ(int(total_src_bytes)), SZ(int(n_frames)), SZ(int(total_blocks)), C.c_uint(_align_log(align_log))))
        if r >= (1 << 62):
            raise ValueError("frame_packed_bound(%r, %r, %r, %r)" % (total_src_bytes, n_frames, total_blocks, align_log))
        return r

    def _check_packed_guard(g, doff, res, n, what):
        """guard mode of the packed writers: nothing behind the capacity, and nothing between the frames -- the writer's contract is the frames'
        bytes and nothing else, the padding included (include/fsehip.h)"""
        g.check(what)
        total = int(doff[n].item())
        if total:
            idx = torch.arange(total, device=doff.device)
            slot = torch.searchsorted(doff[1:n + 1].contiguous(), idx, right=True).clamp(max=n - 1)
            beyond = (idx - doff[slot]) >= res[slot].clamp(min=0)
            assert bool((g.full[0, :total][beyond] == g.fill).all()), "%s wrote outside a frame's bytes" % what

    def frame_compress_packed_dbatch(self, src, src_offsets, block_size_id=5, codec=0, dst=None, capacity=None, max_total_blocks=None, align_log=0, dst_offsets=None,
                                     workspace=None, results=None):
        """-> (dst, dst_offsets, results): frame i = dst[dst_offsets[i] : dst_offsets[i] + results[i]], the frames back to back with every start
        rounded up to 1 << align_log; dst_offsets (int64, n + 1 entries) comes from the device and is what frame_decompress_packed_dbatch takes
        as frame_offsets.  `capacity` defaults to dst's size; dst None: a destination (guarded in guard mode) of `capacity` bytes, by default
        frame_packed_bound(...) of the contents, which no frame can miss.  A frame the capacity cuts short gets -2 (dstSize_tooSmall) and is not
        written.  With dst, max_total_blocks, dst_offsets, workspace and results given the call is launches only and can be captured into a graph."""
        align_log = _align_log(align_log)
        _flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, max_total_blocks is None or (dst is None and capacity is None))
        n = soff.numel() - 1
        if shost is not None:
            blocks = sum(self.frame_block_count(int(x), block_size_id) for x in np.diff(shost)) if block_size_id <= 6 else 0
        if max_total_blocks is None:
            max_total_blocks = blocks
        g = None
        if dst is None:
            if capacity is None:
                capacity = self.frame_packed_bound(int(shost[-1] - shost[0]), n, blocks, align_log)
            dst, g = self._dst(1, int(capacity), src.device)
            dst = dst[0]
        else:
            _flat(dst, "dst")
            capacity = dst.numel() if capacity is None else int(capacity)
            if capacity > dst.numel():
                raise ValueError("capacity %d: dst holds %d bytes" % (capacity, dst.numel()))
        doff = torch.empty(n + 1, dtype=torch.int64, device=src.device) if dst_offsets is None else dst_offsets
        res = torch.zeros(max(n, 1), dtype=torch.int64, device=src.device)[:n] if results is None else results
        if workspace is None:
            self.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = SZ
            need = int(self.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(n), SZ(max_total_blocks), C.c_uint(min(block_size_id, 6)),
                                                                                  C.c_int(codec if codec in (0, 1) else 0)))
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
        _check(self.lib.FSEHIP_frame_compress_packed_dbatch(_ptr(dst), C.c_uint64(int(capacity)), _ptr(doff), _ptr(res), _ptr(src), _ptr(soff), SZ(n),
                                                            SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(codec), C.c_uint(align_log),
                                                            _ptr(workspace), SZ(workspace.numel()), _stream()), "frame_compress_packed_dbatch")
        if g is not None:
            _check_packed_guard(g, doff, res, n, "frame_compress_packed_dbatch")
        return dst, doff, res

    # ---- the packed writer with a codec per frame (fsehip.h, FSEHIP_frame_compress_packed_mixed_dbatch): given, or chosen by size
    def frame_mixed_workspace_bound(self, n_frames, max_total_blocks, block_size_id=5, choose=True):
        """the workspace of frame_compress_packed_mixed_dbatch (choose: the CHOOSE policy, else GIVEN).  Host arithmetic: needs no device."""
        self.lib.FSEHIP_frame_mixedWorkspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_frame_mixedWorkspaceBound(SZ(int(n_frames)), SZ(int(max_total_blocks)), C.c_uint(block_size_id),
                                                          C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN)))
        if r >= (1 << 62):
            raise ValueError("frame_mixed_workspace_bound(%r, %r, %r)" % (n_frames, max_total_blocks, block_size_id))
        return r

    def frame_compress_packed_mixed_dbatch(self, src, src_offsets, codecs=None, tolerance_permille=0, block_size_id=5, dst=None, capacity=None, max_total_blocks=None,
                                           align_log=0, dst_offsets=None, workspace=None, results=None):
        """-> (dst, dst_offsets, results, codecs): frame_compress_packed_dbatch with a codec per frame.  `codecs` given (a CUDA uint8 tensor of
        n entries, 0 = FSE, 1 = Huff0): frame i is written with codecs[i] (any other value: -1 for that frame, which takes no room); the tensor
        is returned as it is.  codecs None: every block goes through both coders and frame i becomes Huff0 unless its Huff0 frame is more than
        tolerance_permille / 1000 larger than its FSE frame; the tensor returned is the choice.  A steady workload chooses once and hands the
        codecs back in afterwards.  Everything else is frame_compress_packed_dbatch's."""
        align_log = _align_log(align_log)
        _flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, max_total_blocks is None or (dst is None and capacity is None))
        n = soff.numel() - 1
        choose = codecs is None
        if choose:
            if not isinstance(tolerance_permille, numbers.Integral) or not 0 <= tolerance_permille <= 1000:
                raise ValueError("tolerance_permille %r: 0 .. 1000" % (tolerance_permille,))
            cgu = _Guarded(1, n, self.guard, src.device) if self.guard > 0 else None
            codecs = cgu.view[0] if cgu is not None else torch.empty(max(n, 1), dtype=torch.uint8, device=src.device)
        else:
            cgu = None
            if not isinstance(codecs, torch.Tensor) or not codecs.is_cuda or codecs.dtype != torch.uint8 or not codecs.is_contiguous() or codecs.numel() != n:
                raise TypeError("codecs must be a contiguous CUDA uint8 tensor of %d entries" % n)
        if shost is not None:
            blocks = sum(self.frame_block_count(int(x), block_size_id) for x in np.diff(shost)) if block_size_id <= 6 else 0
        if max_total_blocks is None:
            max_total_blocks = blocks
        g = None
        if dst is None:
            if capacity is None:
                capacity = self.frame_packed_bound(int(shost[-1] - shost[0]), n, blocks, align_log)
            dst, g = self._dst(1, int(capacity), src.device)
            dst = dst[0]
        else:
            _flat(dst, "dst")
            capacity = dst.numel() if capacity is None else int(capacity)
            if capacity > dst.numel():
                raise ValueError("capacity %d: dst holds %d bytes" % (capacity, dst.numel()))
        doff = torch.empty(n + 1, dtype=torch.int64, device=src.device) if dst_offsets is None else dst_offsets
        res = torch.zeros(max(n, 1), dtype=torch.int64, device=src.device)[:n] if results is None else results
        if workspace is None:
            workspace = torch.empty(max(self.frame_mixed_workspace_bound(n, max_total_blocks, min(block_size_id, 6), choose), 1), dtype=torch.uint8, device=src.device)
        _check(self.lib.FSEHIP_frame_compress_packed_mixed_dbatch(_ptr(dst), C.c_uint64(int(capacity)), _ptr(doff), _ptr(res), _ptr(src), _ptr(soff), SZ(n),
                                                                  SZ(max_total_blocks), C.c_uint(block_size_id), _ptr(codecs if codecs.numel() else codecs.new_zeros(1)),
                                                                  C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(int(tolerance_permille) if choose else 0),
                                                                  C.c_uint(align_log), _ptr(workspace), SZ(workspace.numel()), _stream()),
               "frame_compress_packed_mixed_dbatch")
        if cgu is not None:
            cgu.check("frame_compress_packed_mixed_dbatch (codecs)")
            assert n == 0 or bool((cgu.view[0, :n] <= 1).all()), "frame_compress_packed_mixed_dbatch did not write every codec"
        if g is not None:
            _check_packed_guard(g, doff, res, n, "frame_compress_packed_mixed_dbatch")
        return dst, doff, res, codecs[:n]

    FseHip._flat = staticmethod(_flat)
    for f in (_offsets, frame_block_count, frame_dbatch_plan, frame_dbatch_workspace, xxh32_batch, frame_compress_dbatch, frame_decompress_dbatch,
              frame_inspect, frame_plan_dbatch, frame_decompress_packed_dbatch, frame_packed_bound, frame_compress_packed_dbatch,
              frame_mixed_workspace_bound, frame_compress_packed_mixed_dbatch):
        setattr(FseHip, f.__name__, f)


_frame_dev_methods()


# ---------------------------------------------------------------------------------------------------------
#  Byte planes of tensors (csrc/planes.hip; fsehip.h "byte planes of tensors"): tensors of 1-, 2-, 4- and 8-byte elements, one frame per plane
# ---------------------------------------------------------------------------------------------------------
class CompressedTensors:
    """What compress_tensors returns: per group of tensors of one element size the packed frames (a CUDA uint8 tensor cut to their real total),
    their offsets and results and the split's tensor results (CUDA int64 tensors), and per tensor its dtype, shape and device.  `delta`: the
    frames hold `tensor XOR base` (compress_tensors with base=...) and decompress_tensors needs the same base again; the frames themselves do
    not say so.  `segment_log` (None, or the integer compress_tensors_segmented set): every plane is cut into segments of 1 << segment_log
    bytes with a frame each; frame_offsets, frame_results and codecs are then per segment and every group carries `seg_first` (numpy uint64,
    the first segment of every plane and the segment count).  `delta_op` ("xor", or "sub" where compress_tensors was given a
    DeltaBase(..., "sub")): what the frames of an object with `delta` set hold -- `tensor XOR base` or zigzag(tensor - base); the reading
    calls take it from here.  `sparse_permille` (None, or the integer of the SparsePlanes the object was written with): the frames hold sparse
    contents -- `codec` is then that SparsePlanes -- and decompress_tensors reads them as such; windows and patches of such an object are
    refused.  `transforms` (None, or one name per tensor out of "plain", "pred", "xor", "sub" where compress_tensors_each wrote the object): every
    tensor's planes are those of its own transform, and decompress_tensors merges each accordingly (a base only where a name is "xor" or
    "sub"); decompress_tensor_windows_each and patch_tensor_windows_each take such an object.  `strides` (None, or one integer 1 .. 8 per tensor where
    compress_tensors_each was given `strides`): the stride of every "pred" tensor, 1 for the others; an object that holds one above 1 has no
    windows and no patches.  `base_digests` (None, or one int per tensor in tensor order where the object was written against a DeltaBase(..., check=True)):
    the 64-bit digests of the base tensors; decompress_tensors refuses a base whose digests differ.  `predictor` (None, or "prev" where the
    object was written with a PredictedPlanes -- `codec` is then that PredictedPlanes): the frames hold the planes of the neighbour
    differences, and decompress_tensors sums them back; decompress_tensor_windows_each and patch_tensor_windows_each take such an object."""
    segment_log = None
    delta_op = "xor"
    sparse_permille = None
    base_digests = None
    predictor = None
    transforms = None
    strides = None

    def __init__(self, groups, dtypes, shapes, device, codec, block_size_id, delta=False):
        self.groups, self.dtypes, self.shapes, self.device, self.codec, self.block_size_id = groups, dtypes, shapes, device, codec, block_size_id
        self.delta = bool(delta)

    @property
    def nbytes(self):
        """bytes of all frames"""
        return sum(int(g["frames"].numel()) for g in self.groups)


EST_NAMES = ("plain", "pred", "xor", "sub")      # FSEHIP_EST_PLAIN / _PRED / _XOR / _SUB (include/fsehip.h, "plane estimates"): candidate id = position


class TensorBundle:
    """What compress_tensors_auto returns: the tensors of a mixed list, each compressed with the plane transform chosen for it from the
    device estimates (include/fsehip.h "plane estimates").  `parts` maps the transform name ("plain", "pred", "xor", "sub"; only those
    that were chosen) to an ordinary CompressedTensors -- what compress_tensors returns for that part, and what archive_tensors /
    save_tensors take; `index` maps the same names to the positions of the part's tensors in the input list (every position in exactly one
    part); `estimates` holds one record per input tensor, as estimate_tensors returns them.  decompress_tensors takes the bundle and, where
    it holds an "xor" or a "sub" part, the base of the whole list."""

    def __init__(self, parts, index, estimates, n_tensors):
        self.parts, self.index, self.estimates, self.n_tensors = parts, index, estimates, int(n_tensors)

    @property
    def nbytes(self):
        """bytes of all frames of all parts"""
        return sum(p.nbytes for p in self.parts.values())


class ArchiveInfo(C.Structure):
    """FSEHIP_ArchiveInfo (include/fsehip.h, "tensor archives"): the 64 header bytes of an archive as they lie in it, and headBytes"""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint16), ("flags", C.c_uint16), ("elemBytes", C.c_uint8), ("blockSizeId", C.c_uint8), ("segLog", C.c_uint8),
                ("deltaOp", C.c_uint8), ("sparsePermille", C.c_uint16), ("reserved", C.c_uint16), ("nTensors", C.c_uint64), ("nFrames", C.c_uint64),
                ("totalBytes", C.c_uint64), ("maxTotalBlocks", C.c_uint64), ("metaBytes", C.c_uint64), ("framesBytes", C.c_uint64), ("headBytes", C.c_uint64)]


ARCHIVE_MAGIC, ARCHIVE_VERSION = 0x41545346, 1                                       # the bytes F S T A
ARCHIVE_CODECS, ARCHIVE_DIGESTS, ARCHIVE_SPARSE, ARCHIVE_DELTA = 1, 2, 4, 8          # FSEHIP_ARCHIVE_* (include/fsehip.h)


def _planes_methods():
    def _elem(elem_bytes):
        if elem_bytes not in (1, 2, 4, 8):
            raise TypeError("element size %r: planes are cut for elements of 1, 2, 4 or 8 bytes" % (elem_bytes,))
        return int(elem_bytes)

    def _align_log(align_log):
        if not isinstance(align_log, numbers.Integral) or not 0 <= align_log <= 12:
            raise ValueError("align_log %r: slots are aligned to 1 << 0 .. 1 << 12 bytes" % (align_log,))
        return int(align_log)

    def _i64(self, t, n, device, what):
        if t is None:
            return torch.zeros(max(n, 1), dtype=torch.int64, device=device)[:n]
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < n:
            raise TypeError("%s must be a contiguous CUDA int64 tensor of at least %d entries" % (what, n))
        return t

    def _room(self, t, capacity, what):
        """a caller's flat buffer and the capacity handed to the library for it"""
        self._flat(t, what)
        capacity = t.numel() if capacity is None else int(capacity)
        if capacity > t.numel():
            raise ValueError("capacity %d: %s holds %d bytes" % (capacity, what, t.numel()))
        return capacity

    def planes_block_bound(self, total_bytes, n_tensors, elem_bytes, block_size_id=5):
        """a sufficient max_total_blocks for the planes of n_tensors tensors of total_bytes bytes in all.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_planes_blockBound.restype = SZ
        r = int(self.lib.FSEHIP_planes_blockBound(SZ(int(total_bytes)), SZ(int(n_tensors)), C.c_uint(elem_bytes), C.c_uint(block_size_id)))
        if r >= (1 << 62):
            raise ValueError("planes_block_bound(%r, %r, %r, %r)" % (total_bytes, n_tensors, elem_bytes, block_size_id))
        return r

    def _base(self, base, like, capacity, what):
        """the base of an XOR call (None: a plain call, nothing to check): a flat buffer on the device of `like` that holds at least the
        capacity of the buffer it is laid out as"""
        if base is None:
            return None
        self._flat(base, "base")
        if base.device != like.device:
            raise ValueError("base is on %s, %s on %s" % (base.device, what, like.device))
        if base.numel() < capacity:
            raise ValueError("base holds %d bytes, the capacity of %s is %d" % (base.numel(), what, capacity))
        return base

    def _delta_op(delta_op):
        """the `delta_op` of a call that takes a base: 0 / "xor" or 1 / "sub" (FSEHIP_DELTA_XOR / FSEHIP_DELTA_SUB) -> 0 or 1"""
        if isinstance(delta_op, str) and delta_op in DELTA_OPS:
            return DELTA_OPS[delta_op]
        if isinstance(delta_op, numbers.Integral) and not isinstance(delta_op, bool) and delta_op in (0, 1):
            return int(delta_op)
        raise ValueError("delta_op %r: 0 (\"xor\") or 1 (\"sub\")" % (delta_op,))

    def _call_base(self, name, op, at, *args):
        """the C call `name`, whose d_base is args[at]: itself for XOR, else its *_op_dbatch sibling with deltaOp behind d_base"""
        if not op:
            return getattr(self.lib, name)(*args)
        return getattr(self.lib, name.replace("_xor_", "_").replace("_dbatch", "_op_dbatch"))(*args[:at + 1], C.c_uint(op), *args[at + 1:])

    # ---- what the compress wrappers set up alike ...
    def _codecs(self, codecs, n_frames, device):
        """-> (codecs, guard): the codecs argument of a mixed writer for n_frames frames -- given, or None: an array for the library to fill"""
        if codecs is None:
            g = _Guarded(1, n_frames, self.guard, device) if self.guard > 0 else None
            return (g.view[0] if g is not None else torch.empty(max(n_frames, 1), dtype=torch.uint8, device=device)), g
        if not isinstance(codecs, torch.Tensor) or not codecs.is_cuda or codecs.dtype != torch.uint8 or not codecs.is_contiguous() or codecs.numel() != n_frames:
            raise TypeError("codecs must be a contiguous CUDA uint8 tensor of %d entries" % n_frames)
        return codecs, None

    def _check_codecs(g, n_frames, what):
        if g is not None:
            g.check(what + " (codecs)")
            assert n_frames == 0 or bool((g.view[0, :n_frames] <= 1).all()), what + " did not write every codec"

    def _frames_room(self, shost, n, E, n_frames, block_size_id, max_total_blocks, dst, dst_capacity, align_log, device):
        """-> (max_total_blocks, dst, dst_capacity, guard): the block bound of the planes and the room for n_frames frames of them"""
        if shost is not None:
            blocks = self.planes_block_bound(int(shost[-1] - shost[0]), n, E, min(block_size_id, 6))
        if max_total_blocks is None:
            max_total_blocks = blocks
        if dst is not None:
            return max_total_blocks, dst, _room(self, dst, dst_capacity, "dst"), None
        if dst_capacity is None:
            dst_capacity = self.frame_packed_bound(int(shost[-1] - shost[0]), n_frames, blocks, align_log)
        dst, g = self._dst(1, int(dst_capacity), device)
        return max_total_blocks, dst[0], dst_capacity, g

    def _split_room(self, planes, src, capacity, needed):
        """the planes buffer of a split: the caller's, which must hold `capacity` bytes, or (where the split writes one) as large as src"""
        if planes is None and needed:
            return torch.empty(max(src.numel(), 1), dtype=torch.uint8, device=src.device)
        if planes is not None and _room(self, planes, None, "planes") < capacity:
            raise ValueError("planes holds %d bytes, the capacity is %d" % (planes.numel(), capacity))
        return planes

    def _writer_need(self, n_frames, max_total_blocks, block_size_id, codec, mixed, choose):
        if mixed:
            return self.frame_mixed_workspace_bound(n_frames, max_total_blocks, min(block_size_id, 6), choose)
        self.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = SZ
        return int(self.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(SZ(n_frames), SZ(max_total_blocks), C.c_uint(min(block_size_id, 6)),
                                                                              C.c_int(codec if codec in (0, 1) else 0)))

    def _writer_workspace(self, workspace, n_frames, max_total_blocks, block_size_id, codec, mixed, choose, device):
        if workspace is not None:
            return workspace
        return torch.empty(max(_writer_need(self, n_frames, max_total_blocks, block_size_id, codec, mixed, choose), 1), dtype=torch.uint8, device=device)

    # ---- ... and the merge and decompress wrappers
    def _dst_room(self, dst, capacity, dhost, device):
        """-> (dst, capacity, guard): the caller's destination, or one of `capacity` (default: the end of the last slot) bytes"""
        if dst is not None:
            return dst, _room(self, dst, capacity, "dst"), None
        capacity = int(dhost[-1]) if capacity is None else int(capacity)
        dst, g = self._dst(1, capacity, device)
        return dst[0], capacity, g

    def _planes_room(self, planes, planes_capacity, default, device):
        """-> (planes, planes_capacity): the caller's scratch for the decoded planes, or one of planes_capacity (default: `default`) bytes"""
        if planes is not None:
            return planes, _room(self, planes, planes_capacity, "planes")
        planes_capacity = default if planes_capacity is None else int(planes_capacity)
        return torch.empty(max(planes_capacity, 1), dtype=torch.uint8, device=device), planes_capacity

    def _reader_need(self, n_frames, max_total_blocks):
        self.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = SZ
        return int(self.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(n_frames), SZ(max_total_blocks)))

    def _reader_workspace(self, workspace, n_frames, max_total_blocks, device):
        if workspace is not None:
            return workspace
        return torch.empty(max(_reader_need(self, n_frames, max_total_blocks), 1), dtype=torch.uint8, device=device)

    def planes_split_dbatch(self, src, src_offsets, elem_bytes, capacity=None, planes=None, plane_offsets=None, results=None):
        """-> (planes, plane_offsets, results): tensor i = src[src_offsets[i] : src_offsets[i+1]]; plane p of it (its bytes p, p + E, ..) =
        planes[plane_offsets[i*E+p] : plane_offsets[i*E+p+1]]; results[i] = its size, or -1 (GENERIC) for a tensor that ends behind `capacity`
        (default: src's size).  elem_bytes 1: no kernel over the data, `planes` is src itself unless one is given (it is not written).  With
        src_offsets on the device and planes, plane_offsets and results given the call is launches only and can be captured into a graph."""
        return _split(self, src, None, src_offsets, elem_bytes, capacity, planes, plane_offsets, results)

    def planes_split_xor_dbatch(self, src, base, src_offsets, elem_bytes, capacity=None, planes=None, plane_offsets=None, results=None, delta_op=0):
        """planes_split_dbatch of src XOR base, the XOR fused into the split: `base` is laid out as src is (the same offsets, at least `capacity`
        bytes).  For every elem_bytes, 1 included, `planes` is a buffer of its own and is written; it overlaps neither src nor base.
        delta_op 1 ("sub"): the planes of zigzag(src - base) instead (FSEHIP_planes_split_op_dbatch)."""
        if base is None:
            raise ValueError("planes_split_xor_dbatch needs a base")
        return _split(self, src, base, src_offsets, elem_bytes, capacity, planes, plane_offsets, results, _delta_op(delta_op))

    def _split(self, src, base, src_offsets, elem_bytes, capacity, planes, plane_offsets, results, op=0):
        E = _elem(elem_bytes)
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        what = "planes_split_dbatch" if base is None else "planes_split_xor_dbatch"
        _base(self, base, src, capacity, "src")
        g = None
        if planes is None:
            if E == 1 and base is None:
                planes = src
            else:
                planes, g = self._dst(1, src.numel(), src.device)
                planes = planes[0]
        elif _room(self, planes, None, "planes") < capacity:
            raise ValueError("planes holds %d bytes, the capacity is %d" % (planes.numel(), capacity))
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        res = _i64(self, results, n, src.device, "results")
        if base is None:
            _check(self.lib.FSEHIP_planes_split_dbatch(VP(0) if E == 1 else _ptr(planes), _ptr(poff), _ptr(res), _ptr(src), _ptr(soff), SZ(n), C.c_uint(E),
                                                       C.c_uint64(capacity), _stream()), what)
        else:
            _check(_call_base(self, "FSEHIP_planes_split_xor_dbatch", op, 4, _ptr(planes), _ptr(poff), _ptr(res), _ptr(src), _ptr(base), _ptr(soff), SZ(n), C.c_uint(E),
                              C.c_uint64(capacity), _stream()), what)
        if g is not None:
            g.check(what)
        return planes, poff, res

    def planes_merge_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, dst=None, capacity=None, results=None):
        """-> (dst, results): the inverse of planes_split_dbatch.  Tensor i is rebuilt at dst[dst_offsets[i]:], its slot up to dst_offsets[i+1];
        plane_offsets / plane_sizes (n * E entries are read of each) are what frame_decompress_packed_dbatch returns as dst_offsets / results:
        negative sizes are error codes and become the tensor's result.  results[i] = the tensor's size, or -1 (slot behind `capacity`, default
        dst's size), a plane's error, -4 (sizes that are not the planes of one tensor), -2 (slot too small): such a tensor is not written."""
        return _merge(self, planes, plane_offsets, plane_sizes, None, dst_offsets, elem_bytes, dst, capacity, results)

    def planes_merge_xor_dbatch(self, planes, plane_offsets, plane_sizes, base, dst_offsets, elem_bytes, dst=None, capacity=None, results=None, delta_op=0):
        """planes_merge_dbatch, every rebuilt tensor XORed with `base`, which is laid out as dst is (dst_offsets, at least `capacity` bytes): the
        inverse of planes_split_xor_dbatch.  dst may be `base` itself -- IN PLACE: base then holds the new tensors, and a tensor whose result is
        an error keeps its old bytes.  Any other overlap of dst and base is an error of the caller's that is not checked.
        delta_op 1 ("sub"): base + unzigzag(the rebuilt tensor) instead (FSEHIP_planes_merge_op_dbatch), in place too."""
        if base is None:
            raise ValueError("planes_merge_xor_dbatch needs a base")
        return _merge(self, planes, plane_offsets, plane_sizes, base, dst_offsets, elem_bytes, dst, capacity, results, _delta_op(delta_op))

    def _merge(self, planes, plane_offsets, plane_sizes, base, dst_offsets, elem_bytes, dst, capacity, results, op=0):
        E = _elem(elem_bytes)
        self._flat(planes, "planes")
        doff, dhost = self._offsets(dst_offsets, planes.device, dst is None)
        n = doff.numel() - 1
        poff = _i64(self, plane_offsets, n * E, planes.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, planes.device, "plane_sizes")
        dst, capacity, g = _dst_room(self, dst, capacity, dhost, planes.device)
        res = _i64(self, results, n, planes.device, "results")
        if base is None:
            what = "planes_merge_dbatch"
            _check(self.lib.FSEHIP_planes_merge_dbatch(_ptr(dst), _ptr(doff), _ptr(res), _ptr(planes), _ptr(poff), _ptr(psz), SZ(n), C.c_uint(E), C.c_uint64(capacity),
                                                       _stream()), what)
        else:
            what = "planes_merge_xor_dbatch"
            _base(self, base, planes, capacity, "dst")
            _check(_call_base(self, "FSEHIP_planes_merge_xor_dbatch", op, 6, _ptr(dst), _ptr(doff), _ptr(res), _ptr(planes), _ptr(poff), _ptr(psz), _ptr(base), SZ(n),
                              C.c_uint(E), C.c_uint64(capacity), _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    def tensor_compress_dbatch(self, src, src_offsets, elem_bytes, block_size_id=5, codec=0, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None,
                               align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None, plane_offsets=None, workspace=None):
        """-> (dst, frame_offsets, frame_results, tensor_results): planes_split_dbatch, then frame_compress_packed_dbatch over the planes --
        frame i*E+p = dst[frame_offsets[i*E+p] : .. + frame_results[i*E+p]] is the .fse frame of plane p of tensor i.  `capacity` (default:
        src's size) bounds the tensors, `dst_capacity` (default: dst's size; dst None: frame_packed_bound of the planes) the frames.  planes
        (src.numel() bytes) and plane_offsets (n*E+1) are scratch; the workspace is the packed writer's for n*E frames.  With everything given
        and src_offsets on the device the call is launches only and can be captured into a graph."""
        return _compress(self, src, None, src_offsets, elem_bytes, block_size_id, codec, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                         frame_results, tensor_results, planes, plane_offsets, workspace)

    def tensor_compress_delta_dbatch(self, src, base, src_offsets, elem_bytes, block_size_id=5, codec=0, capacity=None, dst=None, dst_capacity=None,
                                     max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None, plane_offsets=None,
                                     workspace=None, delta_op=0):
        """tensor_compress_dbatch of src XOR base (planes_split_xor_dbatch, then the packed writer over the planes): frame i*E+p is the .fse frame
        of plane p of tensor_i XOR base_i.  `base` is laid out as src is.  `planes` is scratch for every elem_bytes, 1 included.
        delta_op 1 ("sub"): of zigzag(tensor_i - base_i) instead (FSEHIP_tensor_compress_delta_op_dbatch)."""
        if base is None:
            raise ValueError("tensor_compress_delta_dbatch needs a base")
        return _compress(self, src, base, src_offsets, elem_bytes, block_size_id, codec, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                         frame_results, tensor_results, planes, plane_offsets, workspace, op=_delta_op(delta_op))

    def tensor_compress_mixed_dbatch(self, src, src_offsets, elem_bytes, base=None, codecs=None, tolerance_permille=0, block_size_id=5, capacity=None, dst=None,
                                     dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None,
                                     plane_offsets=None, workspace=None, delta_op=0):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs): tensor_compress_dbatch (base None) or tensor_compress_delta_dbatch with
        a codec per plane, as frame_compress_packed_mixed_dbatch has it: `codecs` (a CUDA uint8 tensor of n*E entries, entry i*E+p for plane p of
        tensor i) is given, or None -- then chosen by size at tolerance_permille and returned.  The workspace is the mixed writer's
        (frame_mixed_workspace_bound for n*E frames).  delta_op: what a base means, 0 ("xor") or 1 ("sub")."""
        return _compress(self, src, base, src_offsets, elem_bytes, block_size_id, None, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                         frame_results, tensor_results, planes, plane_offsets, workspace, mixed=(codecs, tolerance_permille), op=_delta_op(delta_op))

    def _compress(self, src, base, src_offsets, elem_bytes, block_size_id, codec, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                  frame_results, tensor_results, planes, plane_offsets, workspace, mixed=None, op=0):
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        self._flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, max_total_blocks is None or (dst is None and dst_capacity is None))
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        what = "tensor_compress_mixed_dbatch" if mixed is not None else "tensor_compress_dbatch" if base is None else "tensor_compress_delta_dbatch"
        _base(self, base, src, capacity, "src")
        choose = False
        if mixed is not None:
            codecs, tol = mixed
            choose = codecs is None
            if choose and (not isinstance(tol, numbers.Integral) or not 0 <= tol <= 1000):
                raise ValueError("tolerance_permille %r: 0 .. 1000" % (tol,))
            codecs, cgu = _codecs(self, codecs, n * E, src.device)
        max_total_blocks, dst, dst_capacity, g = _frames_room(self, shost, n, E, n * E, block_size_id, max_total_blocks, dst, dst_capacity, align_log, src.device)
        planes = _split_room(self, planes, src, capacity, E > 1 or base is not None)
        foff = _i64(self, frame_offsets, n * E + 1, src.device, "frame_offsets")
        fres = _i64(self, frame_results, n * E, src.device, "frame_results")
        tres = _i64(self, tensor_results, n, src.device, "tensor_results")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        workspace = _writer_workspace(self, workspace, n * E, max_total_blocks, block_size_id, codec, mixed is not None, choose, src.device)
        if mixed is not None:
            _check(_call_base(self, "FSEHIP_tensor_compress_mixed_dbatch", op, 6, _ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src),
                              _ptr(base), _ptr(soff), SZ(n), C.c_uint(E), C.c_uint64(capacity), SZ(max_total_blocks), C.c_uint(block_size_id),
                              _ptr(codecs if codecs.numel() else codecs.new_zeros(1)), C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN),
                              C.c_uint(int(tol) if choose else 0), C.c_uint(align_log), _ptr(planes), _ptr(poff), _ptr(workspace), SZ(workspace.numel()), _stream()), what)
            _check_codecs(cgu, n * E, what)
            if g is not None:
                g.check(what)
            return dst, foff, fres, tres, codecs[:n * E]
        tail = (SZ(n), C.c_uint(E), C.c_uint64(capacity), SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(codec), C.c_uint(align_log), _ptr(planes), _ptr(poff),
                _ptr(workspace), SZ(workspace.numel()), _stream())
        if base is None:
            _check(self.lib.FSEHIP_tensor_compress_dbatch(_ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src), _ptr(soff), *tail), what)
        else:
            _check(_call_base(self, "FSEHIP_tensor_compress_delta_dbatch", op, 6, _ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src),
                              _ptr(base), _ptr(soff), *tail), what)
        if g is not None:
            g.check(what)
        return dst, foff, fres, tres

    def tensor_decompress_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, dst=None, dst_capacity=None, max_total_blocks=None, planes=None,
                                 planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None, results=None):
        """-> (dst, results): frame_decompress_packed_dbatch of the n*E frames into `planes`, then planes_merge_dbatch into the slots dst_offsets
        (n + 1 entries, an input).  results[i] = the tensor's size, or the (negative) error of the first of its frames that fails, or the merge's
        own; such a tensor's slot is not written.  planes (default: as many bytes as the slots hold), plane_offsets (n*E+1) and plane_results
        (n*E) are scratch / outputs; the workspace is the packed reader's for n*E frames.  max_total_blocks None: the exact block count of the
        frames, from a frame_plan_dbatch sizing query whose total is read back (planes_block_bound of the tensors is a promise that needs no
        query).  With everything given the call is launches only."""
        return _decompress(self, frames, frame_offsets, None, dst_offsets, elem_bytes, dst, dst_capacity, max_total_blocks, planes, planes_capacity, plane_offsets,
                           plane_results, workspace, results)

    def tensor_decompress_delta_dbatch(self, frames, frame_offsets, base, dst_offsets, elem_bytes, dst=None, dst_capacity=None, max_total_blocks=None, planes=None,
                                       planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None, results=None, delta_op=0):
        """tensor_decompress_dbatch of frames that tensor_compress_delta_dbatch wrote: the packed reader into `planes`, then planes_merge_xor_dbatch
        against `base`, which is laid out as dst is.  dst may be `base` itself (in place): a tensor whose result is an error keeps the base's
        bytes.  delta_op: what the frames were written with, 0 ("xor") or 1 ("sub"); they do not say."""
        if base is None:
            raise ValueError("tensor_decompress_delta_dbatch needs a base")
        return _decompress(self, frames, frame_offsets, base, dst_offsets, elem_bytes, dst, dst_capacity, max_total_blocks, planes, planes_capacity, plane_offsets,
                           plane_results, workspace, results, _delta_op(delta_op))

    def _decompress(self, frames, frame_offsets, base, dst_offsets, elem_bytes, dst, dst_capacity, max_total_blocks, planes, planes_capacity, plane_offsets,
                    plane_results, workspace, results, op=0):
        E = _elem(elem_bytes)
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None or planes is None)
        n = doff.numel() - 1
        if foff.numel() != n * E + 1:
            raise ValueError("frame_offsets: one entry per plane (%d) and one more" % (n * E))
        if max_total_blocks is None:                      # the exact count, from a sizing query (as frame_decompress_packed_dbatch does)
            _, bfirst = self.frame_plan_dbatch(frames, foff, None, 0)
            max_total_blocks = int(bfirst[n * E].item())
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, None if planes is not None else int(dhost[-1]), frames.device)
        poff = _i64(self, plane_offsets, n * E + 1, frames.device, "plane_offsets")
        pres = _i64(self, plane_results, n * E, frames.device, "plane_results")
        res = _i64(self, results, n, frames.device, "results")
        workspace = _reader_workspace(self, workspace, n * E, max_total_blocks, frames.device)
        if base is None:
            what = "tensor_decompress_dbatch"
            _check(self.lib.FSEHIP_tensor_decompress_dbatch(_ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), C.c_uint(E),
                                                            SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(poff), _ptr(pres),
                                                            _ptr(workspace), SZ(workspace.numel()), _stream()), what)
        else:
            what = "tensor_decompress_delta_dbatch"
            _base(self, base, frames, dst_capacity, "dst")
            _check(_call_base(self, "FSEHIP_tensor_decompress_delta_dbatch", op, 3, _ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(base), _ptr(res), _ptr(frames),
                              _ptr(foff), SZ(n), C.c_uint(E), SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(poff), _ptr(pres),
                              _ptr(workspace), SZ(workspace.numel()), _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    # ---- segmented planes (csrc/planes_seg.hip; fsehip.h "segmented planes"): one frame per segment of 1 << segment_log bytes of a plane
    def _seg_log(segment_log, block_size_id=0):
        if not isinstance(segment_log, numbers.Integral) or isinstance(segment_log, bool) or not 10 + block_size_id <= segment_log <= 30:
            raise ValueError("segment_log %r: %d .. 30 (a segment is a whole number of blocks)" % (segment_log, 10 + block_size_id))
        return int(segment_log)

    def planes_segment_first(self, sizes, elem_bytes, segment_log):
        """tensor sizes in bytes -> seg_first (numpy uint64, len(sizes) * E + 1 entries): the index of the first segment of every plane, the last
        entry the number of segments.  A plane of s bytes has max(1, ceil(s / (1 << segment_log))) segments.  Host arithmetic with numpy: needs
        no device.  ValueError for a bad elem_bytes or segment_log, and for 2^31 segments or more."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        n = np.asarray(list(sizes), dtype=np.int64).reshape(-1, 1)
        if n.size and int(n.min()) < 0:
            raise ValueError("sizes: negative")
        p = np.arange(E, dtype=np.int64).reshape(1, -1)
        psize = np.where(n > p, (n - p + E - 1) // E, 0)
        cnt = np.maximum(1, (psize + (1 << L) - 1) >> L).reshape(-1)
        first = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
        if int(first[-1]) >= 1 << 31:
            raise ValueError("planes_segment_first: %d segments, fewer than 2^31 are allowed" % int(first[-1]))
        return first.astype(np.uint64)

    def _seg_first(self, seg_first, n_segments, device, n_planes):
        sf, host = self._offsets(seg_first, device, n_segments is None)
        if sf.numel() != n_planes + 1:
            raise ValueError("seg_first: one entry per plane (%d) and one more" % n_planes)
        return sf, int(host[-1]) if n_segments is None else int(n_segments)

    def planes_segments_dbatch(self, plane_offsets, src_offsets, seg_first, elem_bytes, segment_log, n_segments=None, tensor_results=None, seg_offsets=None):
        """-> (seg_offsets, tensor_results): plane_offsets as planes_split_dbatch leaves them -> the offset of every segment in the planes buffer
        (n_segments + 1 entries: the src_offsets of the packed writers).  A tensor whose counts in seg_first are not those its size implies
        gets -1 in tensor_results (given: updated in place; None: zeros elsewhere) and entries equal to its start.  seg_first on the device
        needs n_segments, else it is read from the host copy."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        poff = plane_offsets
        if not isinstance(poff, torch.Tensor) or not poff.is_cuda or poff.dtype != torch.int64 or not poff.is_contiguous():
            raise TypeError("plane_offsets must be a contiguous CUDA int64 tensor")
        soff, _ = self._offsets(src_offsets, poff.device, False)
        n = soff.numel() - 1
        if poff.numel() < n * E + 1:
            raise ValueError("plane_offsets: one entry per plane (%d) and one more" % (n * E))
        sf, nseg = _seg_first(self, seg_first, n_segments, poff.device, n * E)
        g = None
        if seg_offsets is None:
            seg_offsets, g = self._dst(1, nseg + 1, poff.device, dtype=torch.int64)
            seg_offsets = seg_offsets[0]
        so = _i64(self, seg_offsets, nseg + 1, poff.device, "seg_offsets")
        tres = _i64(self, tensor_results, n, poff.device, "tensor_results")
        _check(self.lib.FSEHIP_planes_segments_dbatch(_ptr(so), _ptr(tres), _ptr(poff), _ptr(soff), _ptr(sf), SZ(n), C.c_uint(E), SZ(nseg), C.c_uint(L), _stream()),
               "planes_segments_dbatch")
        if g is not None:
            g.check("planes_segments_dbatch")
        return so, tres

    def planes_fold_segments_dbatch(self, seg_offsets, seg_results, seg_first, segment_log, n_segments=None, plane_offsets=None, plane_sizes=None):
        """-> (plane_offsets, plane_sizes): what frame_decompress_packed_dbatch returns per segment (dst_offsets, results) -> per plane its
        first segment's offset and its size, or -1 (no segment), the first error among its segments, -4 (segments that are not full, or do not
        lie back to back): what planes_merge_dbatch takes."""
        L = _seg_log(segment_log)
        if not isinstance(seg_offsets, torch.Tensor) or not seg_offsets.is_cuda or seg_offsets.dtype != torch.int64 or not seg_offsets.is_contiguous():
            raise TypeError("seg_offsets must be a contiguous CUDA int64 tensor")
        dev = seg_offsets.device
        sf, host = self._offsets(seg_first, dev, n_segments is None)
        nseg = int(host[-1]) if n_segments is None else int(n_segments)
        npl = sf.numel() - 1
        if seg_offsets.numel() < nseg + 1:
            raise ValueError("seg_offsets: one entry per segment (%d) and one more" % nseg)
        sres = _i64(self, seg_results, nseg, dev, "seg_results")
        g = []
        if plane_offsets is None:
            plane_offsets, x = self._dst(1, npl, dev, dtype=torch.int64)
            plane_offsets = plane_offsets[0]
            g.append(x)
        if plane_sizes is None:
            plane_sizes, x = self._dst(1, npl, dev, dtype=torch.int64)
            plane_sizes = plane_sizes[0]
            g.append(x)
        po = _i64(self, plane_offsets, npl, dev, "plane_offsets")
        ps = _i64(self, plane_sizes, npl, dev, "plane_sizes")
        _check(self.lib.FSEHIP_planes_fold_segments_dbatch(_ptr(po), _ptr(ps), _ptr(seg_offsets), _ptr(sres), _ptr(sf), SZ(npl), SZ(nseg), C.c_uint(L), _stream()),
               "planes_fold_segments_dbatch")
        for x in g:
            if x is not None:
                x.check("planes_fold_segments_dbatch")
        return po[:npl], ps[:npl]

    def tensor_compress_seg_dbatch(self, src, src_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None, base=None, codec=0, codecs=None,
                                   block_size_id=5, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None,
                                   frame_results=None, tensor_results=None, planes=None, plane_offsets=None, seg_offsets=None, workspace=None, delta_op=0):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs): the split (against `base` if one is given, by delta_op), planes_segments_dbatch,
        then the packed writer over the segments -- frame q = dst[frame_offsets[q] : .. + frame_results[q]] is the .fse frame of segment
        q - seg_first[j] of the plane j that holds it.  codec 0 / 1: the packed writer, codecs returned None.  codec an AutoCodec: a codec per
        segment chosen by size and returned; `codecs` (CUDA uint8, one per segment): given.  seg_first None: planes_segment_first of the
        sizes; on the device it needs n_segments.  planes, plane_offsets (n*E+1) and seg_offsets (n_segments+1) are scratch; the workspace is
        the (mixed) writer's for n_segments frames.  With everything given and the offsets on the device the call is launches only."""
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        L = _seg_log(segment_log, min(block_size_id, 6))
        self._flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, seg_first is None or max_total_blocks is None or (dst is None and dst_capacity is None))
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        what = "tensor_compress_seg_dbatch"
        op = _delta_op(delta_op)
        _base(self, base, src, capacity, "src")
        if seg_first is None:
            seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
        sf, nseg = _seg_first(self, seg_first, n_segments, src.device, n * E)
        mixed = codecs is not None or isinstance(codec, AutoCodec)
        choose = mixed and codecs is None
        codecs, cgu = _codecs(self, codecs, nseg, src.device) if mixed else (None, None)
        max_total_blocks, dst, dst_capacity, g = _frames_room(self, shost, n, E, nseg, block_size_id, max_total_blocks, dst, dst_capacity, align_log, src.device)
        planes = _split_room(self, planes, src, capacity, E > 1 or base is not None)
        foff = _i64(self, frame_offsets, nseg + 1, src.device, "frame_offsets")
        fres = _i64(self, frame_results, nseg, src.device, "frame_results")
        tres = _i64(self, tensor_results, n, src.device, "tensor_results")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        so = _i64(self, seg_offsets, nseg + 1, src.device, "seg_offsets")
        workspace = _writer_workspace(self, workspace, nseg, max_total_blocks, block_size_id, codec, mixed, choose, src.device)
        tol = codec.tolerance_permille if choose and isinstance(codec, AutoCodec) else 0
        _check(_call_base(
            self, "FSEHIP_tensor_compress_seg_dbatch", op, 6, _ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src), _ptr(base), _ptr(soff), SZ(n), C.c_uint(E), C.c_uint64(capacity),
            _ptr(sf), SZ(nseg), C.c_uint(L), SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(0 if mixed else codec),
            _ptr((codecs if codecs.numel() else codecs.new_zeros(1)) if mixed else None), C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(tol),
            C.c_uint(align_log), _ptr(planes), _ptr(poff), _ptr(so), _ptr(workspace), SZ(workspace.numel()), _stream()), what)
        _check_codecs(cgu, nseg, what)
        if g is not None:
            g.check(what)
        return dst, foff, fres, tres, (codecs[:nseg] if mixed else None)

    def tensor_decompress_seg_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None, base=None, dst=None,
                                     dst_capacity=None, max_total_blocks=None, planes=None, planes_capacity=None, seg_offsets=None, seg_results=None, plane_offsets=None,
                                     plane_sizes=None, workspace=None, results=None, delta_op=0):
        """-> (dst, results): frame_decompress_packed_dbatch of the n_segments frames into `planes`, planes_fold_segments_dbatch, then the merge
        (against `base` if one is given, by delta_op; dst may be `base` itself) into the slots dst_offsets.  results[i] = the tensor's size, or the error of
        the first of its segments that fails, or the fold's or the merge's own; such a tensor's slot is not written.  seg_first None:
        planes_segment_first of the slots' sizes.  seg_offsets (n_segments+1), seg_results (n_segments), plane_offsets and plane_sizes (n*E
        each) are outputs / scratch; the workspace is the packed reader's for n_segments frames.  max_total_blocks None: the exact count from
        a sizing query whose total is read back."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None or planes is None or seg_first is None)
        n = doff.numel() - 1
        if seg_first is None:
            seg_first = planes_segment_first(self, np.diff(dhost.astype(np.int64)).clip(min=0), E, L)
        sf, nseg = _seg_first(self, seg_first, n_segments, frames.device, n * E)
        if foff.numel() != nseg + 1:
            raise ValueError("frame_offsets: one entry per segment (%d) and one more" % nseg)
        if max_total_blocks is None:
            _, bfirst = self.frame_plan_dbatch(frames, foff, None, 0)
            max_total_blocks = int(bfirst[nseg].item())
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, None if planes is not None else int(dhost[-1]), frames.device)
        so = _i64(self, seg_offsets, nseg + 1, frames.device, "seg_offsets")
        sres = _i64(self, seg_results, nseg, frames.device, "seg_results")
        poff = _i64(self, plane_offsets, n * E, frames.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, frames.device, "plane_sizes")
        res = _i64(self, results, n, frames.device, "results")
        workspace = _reader_workspace(self, workspace, nseg, max_total_blocks, frames.device)
        what = "tensor_decompress_seg_dbatch"
        op = _delta_op(delta_op)
        _base(self, base, frames, dst_capacity, "dst")
        _check(_call_base(
            self, "FSEHIP_tensor_decompress_seg_dbatch", op, 3, _ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(base), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), C.c_uint(E), _ptr(sf), SZ(nseg), C.c_uint(L),
            SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(so), _ptr(sres), _ptr(poff), _ptr(psz), _ptr(workspace), SZ(workspace.numel()),
            _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    # ---- windows of segmented tensors (csrc/planes_win.hip; fsehip.h "windows of segmented tensors"): elements [a, b) of every tensor, decoding
    # only the segments that hold them
    def _window_array(windows, n):
        """(a, b) per tensor as python ints -> numpy int64 of shape (n, 2)"""
        w = np.asarray([(int(a), int(b)) for a, b in windows], dtype=np.int64).reshape(-1, 2)
        if w.shape[0] != n:
            raise ValueError("windows: %d for %d tensors" % (w.shape[0], n))
        return w

    def planes_window_first(self, sizes, windows, elem_bytes, segment_log, block_size_id=5):
        """tensor sizes in bytes and one window (a, b) per tensor, in elements -> (sel_first, max_blocks): sel_first (numpy uint64,
        len(sizes) * E + 1 entries) is the index of the first selected segment frame of every plane, its last entry the number of selected
        frames; max_blocks the exact number of blocks in them, the packed reader's block promise.  Every plane of a tensor contributes the
        segments a >> segment_log .. (b - 1) >> segment_log, none for a == b.  Host arithmetic with numpy: needs no device.  ValueError for a
        bad elem_bytes, block_size_id or segment_log, a window that is not 0 <= a <= b <= size // E, and for 2^31 frames or blocks or more."""
        E = _elem(elem_bytes)
        if not isinstance(block_size_id, numbers.Integral) or not 0 <= block_size_id <= 6:
            raise ValueError("block_size_id %r: 0 .. 6" % (block_size_id,))
        L = _seg_log(segment_log, block_size_id)
        n = np.asarray(list(sizes), dtype=np.int64).reshape(-1)
        w = _window_array(windows, n.size)
        a, b = w[:, 0], w[:, 1]
        if n.size and (int(n.min()) < 0 or bool(((a < 0) | (a > b) | (b > n // E)).any())):
            raise ValueError("planes_window_first: a window is (a, b) in elements with 0 <= a <= b <= size // %d" % E)
        k0 = a >> L
        cnt = np.where(a < b, ((b - 1) >> L) - k0 + 1, 0)
        first = np.concatenate([[0], np.cumsum(np.repeat(cnt, E), dtype=np.int64)])
        p = np.arange(E, dtype=np.int64).reshape(1, -1)
        nn = n.reshape(-1, 1)
        psize = np.where(nn > p, (nn - p + E - 1) // E, 0)
        last = np.minimum(1 << L, psize - ((k0 + cnt - 1).reshape(-1, 1) << L))            # bytes of the last selected segment of every plane
        bl = 10 + int(block_size_id)
        per_plane = (cnt.reshape(-1, 1) - 1) * (1 << (L - bl)) + ((last + (1 << bl) - 1) >> bl)
        blocks = int(np.where(cnt.reshape(-1, 1) > 0, per_plane, 0).sum())
        if int(first[-1]) >= 1 << 31 or blocks >= 1 << 31:
            raise ValueError("planes_window_first: %d frames of %d blocks, fewer than 2^31 are allowed" % (int(first[-1]), blocks))
        return first.astype(np.uint64), blocks

    def _windows(self, windows, device, n):
        """windows on the device as the library takes them: 2 * n int64 (a CUDA int64 tensor of that many entries is taken as it is)"""
        if isinstance(windows, torch.Tensor) and windows.is_cuda:
            if windows.dtype != torch.int64 or not windows.is_contiguous() or windows.numel() != 2 * n:
                raise TypeError("windows must be a contiguous CUDA int64 tensor of %d entries" % (2 * n))
            return windows, None
        w = _window_array(windows.tolist() if isinstance(windows, (torch.Tensor, np.ndarray)) else windows, n)
        return torch.from_numpy(np.ascontiguousarray(w.reshape(-1))).to(device), w

    def _sel_first(self, sel_first, n_selected, device, n_planes):
        wf, host = self._offsets(sel_first, device, n_selected is None)
        if wf.numel() != n_planes + 1:
            raise ValueError("sel_first: one entry per plane (%d) and one more" % n_planes)
        return wf, int(host[-1]) if n_selected is None else int(n_selected)

    def planes_select_window_dbatch(self, frame_offsets, src_offsets, windows, seg_first, sel_first, elem_bytes, segment_log, n_segments=None, n_selected=None,
                                    sel_frame_offsets=None):
        """-> sel_frame_offsets (n_selected + 1 entries): the frame_offsets of the packed reader for the selected segment frames alone -- entry r is
        where selected frame r starts in the frames buffer, extent r runs to the next selected frame (unselected frames included: a reader
        stops at the end mark), the last entry is the end of the last selected frame.  frame_offsets are ALL frames' (n_segments + 1),
        src_offsets the sender's tensor layout, windows one (a, b) in elements per tensor, seg_first / sel_first what planes_segment_first /
        planes_window_first give.  A tensor with a bad window or wrong counts gets empty extents.  seg_first / sel_first on the device need
        n_segments / n_selected."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        foff = frame_offsets
        if not isinstance(foff, torch.Tensor) or not foff.is_cuda or foff.dtype != torch.int64 or not foff.is_contiguous():
            raise TypeError("frame_offsets must be a contiguous CUDA int64 tensor")
        soff, _ = self._offsets(src_offsets, foff.device, False)
        n = soff.numel() - 1
        sf, nseg = _seg_first(self, seg_first, n_segments, foff.device, n * E)
        wf, nsel = _sel_first(self, sel_first, n_selected, foff.device, n * E)
        if foff.numel() < nseg + 1:
            raise ValueError("frame_offsets: one entry per segment (%d) and one more" % nseg)
        win, _ = _windows(self, windows, foff.device, n)
        g = None
        if sel_frame_offsets is None:
            sel_frame_offsets, g = self._dst(1, nsel + 1, foff.device, dtype=torch.int64)
            sel_frame_offsets = sel_frame_offsets[0]
        so = _i64(self, sel_frame_offsets, nsel + 1, foff.device, "sel_frame_offsets")
        _check(self.lib.FSEHIP_planes_select_window_dbatch(_ptr(so), _ptr(foff), _ptr(soff), _ptr(win if n else win.new_zeros(1)), _ptr(sf), _ptr(wf), SZ(n), C.c_uint(E),
                                                           SZ(nseg), SZ(nsel), C.c_uint(L), _stream()), "planes_select_window_dbatch")
        if g is not None:
            g.check("planes_select_window_dbatch")
        return so[:nsel + 1]

    def planes_fold_window_dbatch(self, sel_offsets, sel_results, src_offsets, windows, seg_first, sel_first, elem_bytes, segment_log, n_selected=None,
                                  plane_offsets=None, plane_sizes=None):
        """-> (plane_offsets, plane_sizes), n * E entries each, as planes_merge_dbatch takes them: what frame_decompress_packed_dbatch returns for
        the selected extents (dst_offsets, results) -> per plane where the window's first byte lies and b - a, or -1 (a tensor with a bad
        window or wrong counts), 0 (an empty window), the first error among its selected segments, -4 (a segment that did not regenerate exactly
        its bytes, or segments that do not lie back to back); the offset is 0 unless the size is b - a > 0."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        if not isinstance(sel_offsets, torch.Tensor) or not sel_offsets.is_cuda or sel_offsets.dtype != torch.int64 or not sel_offsets.is_contiguous():
            raise TypeError("sel_offsets must be a contiguous CUDA int64 tensor")
        dev = sel_offsets.device
        soff, _ = self._offsets(src_offsets, dev, False)
        n = soff.numel() - 1
        npl = n * E
        sf, _ = self._offsets(seg_first, dev, False)
        if sf.numel() != npl + 1:
            raise ValueError("seg_first: one entry per plane (%d) and one more" % npl)
        wf, nsel = _sel_first(self, sel_first, n_selected, dev, npl)
        if sel_offsets.numel() < nsel + 1:
            raise ValueError("sel_offsets: one entry per selected frame (%d) and one more" % nsel)
        sres = _i64(self, sel_results, nsel, dev, "sel_results")
        win, _ = _windows(self, windows, dev, n)
        g = []
        if plane_offsets is None:
            plane_offsets, x = self._dst(1, npl, dev, dtype=torch.int64)
            plane_offsets = plane_offsets[0]
            g.append(x)
        if plane_sizes is None:
            plane_sizes, x = self._dst(1, npl, dev, dtype=torch.int64)
            plane_sizes = plane_sizes[0]
            g.append(x)
        po = _i64(self, plane_offsets, npl, dev, "plane_offsets")
        ps = _i64(self, plane_sizes, npl, dev, "plane_sizes")
        _check(self.lib.FSEHIP_planes_fold_window_dbatch(_ptr(po), _ptr(ps), _ptr(sel_offsets), _ptr(sres if nsel else sres.new_zeros(1)), _ptr(soff),
                                                         _ptr(win if n else win.new_zeros(1)), _ptr(sf), _ptr(wf), SZ(n), C.c_uint(E), SZ(nsel), C.c_uint(L), _stream()),
               "planes_fold_window_dbatch")
        for x in g:
            if x is not None:
                x.check("planes_fold_window_dbatch")
        return po[:npl], ps[:npl]

    def tensor_decompress_window_dbatch(self, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None,
                                        sel_first=None, n_selected=None, base=None, dst=None, dst_capacity=None, max_total_blocks=None, block_size_id=5, planes=None,
                                        planes_capacity=None, sel_frame_offsets=None, sel_offsets=None, sel_results=None, plane_offsets=None, plane_sizes=None,
                                        workspace=None, results=None, delta_op=0):
        """-> (dst, results): elements [a, b) of every tensor of a segmented batch -- planes_select_window_dbatch, frame_decompress_packed_dbatch over
        the n_selected extents into `planes`, planes_fold_window_dbatch, then the merge (against `base` if one is given, by delta_op, which holds the same
        windows in dst's layout; dst may be `base` itself) into the slots dst_offsets: slot i receives the E * (b - a) bytes
        tensor_i[a * E : b * E], results[i] is that size or an error, and such a tensor's slot is not written.  src_offsets is the SENDER'S
        layout (the sizes the tensors were compressed with), frame_offsets all n_segments frames'.  seg_first None: planes_segment_first of
        those sizes.  sel_first or max_total_blocks None: planes_window_first of the sizes and windows with `block_size_id` (both then need
        src_offsets and windows on the host).  planes: n_selected << segment_log bytes are always enough (the default).  sel_frame_offsets,
        sel_offsets (n_selected + 1), sel_results (n_selected), plane_offsets and plane_sizes (n * E) are outputs / scratch; the workspace is
        the packed reader's for n_selected frames.  With everything given and on the device the call is launches only.  For frames of
        compress_tensors_segmented with a codec and an optional base; frames written with a transform per tensor or with predicted planes
        go to tensor_decompress_window_each_dbatch."""
        return _window_read(self, "tensor_decompress_window_dbatch", None, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log, seg_first,
                            n_segments, sel_first, n_selected, base, dst, dst_capacity, max_total_blocks, block_size_id, planes, planes_capacity, sel_frame_offsets,
                            sel_offsets, sel_results, plane_offsets, plane_sizes, workspace, results, delta_op)

    def _window_read(self, what, transforms, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log, seg_first, n_segments, sel_first,
                     n_selected, base, dst, dst_capacity, max_total_blocks, block_size_id, planes, planes_capacity, sel_frame_offsets, sel_offsets, sel_results,
                     plane_offsets, plane_sizes, workspace, results, delta_op, stride_call=False, strides=None):
        """the window composites: transforms None -- one op for the batch, delta_op -- or one transform per tensor; stride_call: the
        _each_stride_ export, `strides` as _strides takes them (None: stride 1 everywhere)"""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        need_first = sel_first is None or max_total_blocks is None
        soff, shost = self._offsets(src_offsets, frames.device, seg_first is None or need_first)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None)
        n = soff.numel() - 1
        if doff.numel() != n + 1:
            raise ValueError("dst_offsets: one entry per tensor (%d) and one more" % n)
        win, whost = _windows(self, windows, frames.device, n)
        if seg_first is None:
            seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
        sf, nseg = _seg_first(self, seg_first, n_segments, frames.device, n * E)
        if foff.numel() != nseg + 1:
            raise ValueError("frame_offsets: one entry per segment (%d) and one more" % nseg)
        if need_first:
            if whost is None:
                raise ValueError(what + ": windows on the device need sel_first, n_selected and max_total_blocks")
            first, blocks = planes_window_first(self, np.diff(shost.astype(np.int64)).clip(min=0), whost, E, L, block_size_id)
            sel_first = first if sel_first is None else sel_first
            max_total_blocks = blocks if max_total_blocks is None else max_total_blocks
        wf, nsel = _sel_first(self, sel_first, n_selected, frames.device, n * E)
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, nsel << L, frames.device)
        sfo = _i64(self, sel_frame_offsets, nsel + 1, frames.device, "sel_frame_offsets")
        so = _i64(self, sel_offsets, nsel + 1, frames.device, "sel_offsets")
        sres = _i64(self, sel_results, nsel, frames.device, "sel_results")
        poff = _i64(self, plane_offsets, n * E, frames.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, frames.device, "plane_sizes")
        res = _i64(self, results, n, frames.device, "results")
        workspace = _reader_workspace(self, workspace, nsel, max_total_blocks, frames.device)
        op = _delta_op(delta_op)
        _base(self, base, frames, dst_capacity, "dst")
        tr = None if transforms is None else _transforms(transforms, n, frames.device)
        held = _strides(strides, n, frames.device) if stride_call else None

        def some(t):                                             # (an array of no entries still needs an address)
            return t if t.numel() else t.new_zeros(1)
        head = (_ptr(some(dst)), _ptr(doff), C.c_uint64(dst_capacity), _ptr(base))
        rest = (_ptr(some(res)), _ptr(some(frames)), _ptr(foff), _ptr(soff), _ptr(some(win)), SZ(n),
                C.c_uint(E), _ptr(sf), SZ(nseg), C.c_uint(L), _ptr(wf), SZ(nsel), SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(sfo), _ptr(so),
                _ptr(some(sres)), _ptr(some(poff)), _ptr(some(psz)), _ptr(workspace), SZ(workspace.numel()), _stream())
        if tr is None:
            _check(_call_base(self, "FSEHIP_tensor_decompress_window_dbatch", op, 3, *head, *rest), what)
        elif stride_call:
            _check(self.lib.FSEHIP_tensor_decompress_window_each_stride_dbatch(*head, VP(tr.data_ptr() or res.data_ptr()), _ptr(held), *rest), what)
        else:
            _check(self.lib.FSEHIP_tensor_decompress_window_each_dbatch(*head, VP(tr.data_ptr() or res.data_ptr()), *rest), what)
        if g is not None:
            g.check(what)
        return dst, res

    # ---- patching segmented tensors (csrc/planes_patch.hip; fsehip.h "patching segmented tensors"): the segments that hold a window of every
    # tensor coded anew, the other frames kept
    def _some(t):                                                # (an array of no entries still needs an address)
        return t if t is None or t.numel() else t.new_zeros(1)

    def planes_stage_offsets(self, sizes, windows, elem_bytes, segment_log):
        """tensor sizes in bytes and one window (a, b) per tensor, in elements -> stage_offsets (numpy uint64, len(sizes) + 1 entries): the
        running sum of the bytes of every tensor that its selected segments cover, [k0 * seg * E, min((k0 + cnt) * seg * E, size)) -- where
        planes_split_window_dbatch stages them.  Host arithmetic with numpy: needs no device.  ValueError as planes_window_first."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        n = np.asarray(list(sizes), dtype=np.int64).reshape(-1)
        w = _window_array(windows, n.size)
        a, b = w[:, 0], w[:, 1]
        if n.size and (int(n.min()) < 0 or bool(((a < 0) | (a > b) | (b > n // E)).any())):
            raise ValueError("planes_stage_offsets: a window is (a, b) in elements with 0 <= a <= b <= size // %d" % E)
        k0 = a >> L
        cnt = np.where(a < b, ((b - 1) >> L) - k0 + 1, 0)
        at = (k0 << L) * E
        m = np.where(cnt > 0, np.minimum(n - at, (cnt << L) * E), 0)
        return np.concatenate([[0], np.cumsum(m, dtype=np.int64)]).astype(np.uint64)

    def _split_window(self, what, transforms, src, src_offsets, windows, elem_bytes, segment_log, stage_offsets, base, capacity, stage, stage_capacity, plane_offsets,
                      results, delta_op, stride_call=False, strides=None):
        """planes_split_window_dbatch (transforms None: one op for all), planes_split_window_each_dbatch (a transform per tensor) and, with
        stride_call, planes_split_window_each_stride_dbatch (`strides` as _strides takes them)"""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        soff, shost = self._offsets(src_offsets, src.device, stage_offsets is None)
        n = soff.numel() - 1
        op = 0 if transforms is not None else _delta_op(delta_op)
        tr = None if transforms is None else _transforms(transforms, n, src.device)
        held = _strides(strides, n, src.device) if stride_call else None
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        win, whost = _windows(self, windows, src.device, n)
        if stage_offsets is None:
            if whost is None:
                raise ValueError(what + ": windows on the device need stage_offsets")
            stage_offsets = planes_stage_offsets(self, np.diff(shost.astype(np.int64)).clip(min=0), whost, E, L)
        toff, thost = self._offsets(stage_offsets, src.device, stage is None and stage_capacity is None)
        if toff.numel() != n + 1:
            raise ValueError("stage_offsets: one entry per tensor (%d) and one more" % n)
        g = None
        if stage is None:
            stage_capacity = int(thost[-1]) if stage_capacity is None else int(stage_capacity)
            stage, g = self._dst(1, stage_capacity, src.device)
            stage = stage[0]
        else:
            stage_capacity = _room(self, stage, stage_capacity, "stage")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        res = _i64(self, results, n, src.device, "results")
        args = (_ptr(soff), _ptr(_some(win)), _ptr(toff), SZ(n), C.c_uint(E), C.c_uint(L), C.c_uint64(capacity), C.c_uint64(stage_capacity), _stream())
        if tr is None:
            _check(_call_base(self, "FSEHIP_planes_split_window_dbatch", op, 4, _ptr(stage), _ptr(poff), _ptr(_some(res)), _ptr(_some(src)), _ptr(base), *args), what)
        elif stride_call:
            _check(self.lib.FSEHIP_planes_split_window_each_stride_dbatch(_ptr(stage), _ptr(poff), _ptr(_some(res)), _ptr(_some(src)), _ptr(base),
                                                                          VP(tr.data_ptr() or soff.data_ptr()), _ptr(held), *args), what)
        else:
            _check(self.lib.FSEHIP_planes_split_window_each_dbatch(_ptr(stage), _ptr(poff), _ptr(_some(res)), _ptr(_some(src)), _ptr(base),
                                                                   VP(tr.data_ptr() or soff.data_ptr()), *args), what)
        if g is not None:
            g.check(what)
        return stage, poff, res

    def planes_split_window_dbatch(self, src, src_offsets, windows, elem_bytes, segment_log, stage_offsets=None, base=None, capacity=None, stage=None,
                                   stage_capacity=None, plane_offsets=None, results=None, delta_op=0):
        """-> (stage, plane_offsets, results): per tensor the planes of the bytes its selected segments cover (planes_stage_offsets), staged back to
        back at stage_offsets -- plane p of staged tensor i = stage[plane_offsets[i*E+p] : plane_offsets[i*E+p+1]] is segments k0 .. k1 of plane
        p of the tensor (of tensor XOR base where a base is given, of zigzag(tensor - base) with delta_op 1).  results[i] = the staged bytes, or -1 for a tensor with a bad window, one
        that ends behind `capacity`, or a pair of stage offsets that does not hold exactly those bytes below stage_capacity.  stage_offsets
        None: planes_stage_offsets (src_offsets and windows then on the host); on the device they need stage or stage_capacity."""
        return _split_window(self, "planes_split_window_dbatch", None, src, src_offsets, windows, elem_bytes, segment_log, stage_offsets, base, capacity, stage,
                             stage_capacity, plane_offsets, results, delta_op)

    def planes_splice_scratch_bound(self, n_tensors, elem_bytes, n_segments):
        """bytes of scratch planes_splice_dbatch and tensor_patch_window_dbatch need.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_planes_spliceScratchBound.restype = SZ
        r = int(self.lib.FSEHIP_planes_spliceScratchBound(SZ(int(n_tensors)), C.c_uint(_elem(elem_bytes)), SZ(int(n_segments))))
        if r >= (1 << 62):
            raise ValueError("planes_splice_scratch_bound(%r, %r, %r)" % (n_tensors, elem_bytes, n_segments))
        return r

    def _u8(t, n, device, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < n:
            raise TypeError("%s must be a contiguous CUDA uint8 tensor of at least %d entries" % (what, n))
        return t

    def _splice_out(self, out, out_capacity, default, codecs, out_codecs, nseg, device):
        """-> (out, out_capacity, out_codecs, guards): the caller's output, or one of out_capacity (default: `default`) bytes; the output codecs
        where the object has some"""
        g = []
        if out is None:
            out_capacity = default if out_capacity is None else int(out_capacity)
            out, x = self._dst(1, out_capacity, device)
            out = out[0]
            g.append(x)
        else:
            out_capacity = _room(self, out, out_capacity, "out")
        if codecs is not None and out_codecs is None:
            out_codecs, x = self._dst(1, nseg, device)
            out_codecs = out_codecs[0]
            g.append(x)
        elif out_codecs is not None:
            if codecs is None:
                raise ValueError("out_codecs: the object has no codecs")
            _u8(out_codecs, nseg, device, "out_codecs")
        return out, out_capacity, out_codecs, [x for x in g if x is not None]

    def planes_splice_dbatch(self, frames, frame_offsets, frame_results, new_frames, new_offsets, new_results, src_offsets, windows, seg_first, sel_first,
                             elem_bytes, segment_log, n_segments=None, n_selected=None, codecs=None, new_codecs=None, stage_results=None, frames_capacity=None,
                             new_capacity=None, out=None, out_capacity=None, out_offsets=None, out_results=None, out_codecs=None, tensor_results=None, scratch=None):
        """-> (out, out_offsets, out_results, tensor_results, out_codecs): a new packed object from the frames of an old one (frames,
        frame_offsets n_segments + 1, frame_results, codecs or None) and the new frames of the selected segments (new_frames, new_offsets
        n_selected + 1, new_results, new_codecs iff codecs).  Frame q of the output is new frame sel_first[j] + k - k0 where q is selected
        segment k of plane j, the old frame q otherwise; out_offsets[q + 1] - out_offsets[q] is the new frame's slot or the old extent, and
        only a frame's real bytes are copied.  tensor_results[i] = the tensor's size, or an error: the tensor then keeps ALL its old frames --
        a bad window or wrong counts (-1), an error in stage_results, an old frame that does not lie inside frames_capacity or does not hold
        its result (-4), a new frame with an error (that error).  If the object does not fit out_capacity nothing is written and every
        tensor gets -3; out_offsets are whole even then.  out must not overlap frames or new_frames."""
        E, L = _elem(elem_bytes), _seg_log(segment_log)
        self._flat(frames, "frames")
        dev = frames.device
        foff, _ = self._offsets(frame_offsets, dev, False)
        soff, _ = self._offsets(src_offsets, dev, False)
        n = soff.numel() - 1
        sf, nseg = _seg_first(self, seg_first, n_segments, dev, n * E)
        wf, nsel = _sel_first(self, sel_first, n_selected, dev, n * E)
        if foff.numel() < nseg + 1:
            raise ValueError("frame_offsets: one entry per segment (%d) and one more" % nseg)
        fres = _i64(self, frame_results, nseg, dev, "frame_results")
        if frame_results is None:
            raise TypeError("frame_results: the results of the object's frames are needed")
        frames_capacity = _room(self, frames, frames_capacity, "frames")
        win, _ = _windows(self, windows, dev, n)
        if nsel:
            new_capacity = _room(self, new_frames, new_capacity, "new_frames")
            noff, _ = self._offsets(new_offsets, dev, False)
            if noff.numel() < nsel + 1:
                raise ValueError("new_offsets: one entry per selected frame (%d) and one more" % nsel)
            nres = _i64(self, new_results, nsel, dev, "new_results")
        else:
            new_capacity, noff, nres = 0, None, None
        if codecs is not None:
            _u8(codecs, nseg, dev, "codecs")
            if nsel:
                _u8(new_codecs, nsel, dev, "new_codecs")
        elif new_codecs is not None:
            raise ValueError("new_codecs: the object has no codecs")
        if stage_results is not None:
            _i64(self, stage_results, n, dev, "stage_results")
        out, out_capacity, out_codecs, guards = _splice_out(self, out, out_capacity, frames_capacity + new_capacity, codecs, out_codecs, nseg, dev)
        ooff = _i64(self, out_offsets, nseg + 1, dev, "out_offsets")
        ores = _i64(self, out_results, nseg, dev, "out_results")
        tres = _i64(self, tensor_results, n, dev, "tensor_results")
        if scratch is None:
            scratch = torch.empty(planes_splice_scratch_bound(self, n, E, nseg), dtype=torch.uint8, device=dev)
        what = "planes_splice_dbatch"
        _check(self.lib.FSEHIP_planes_splice_dbatch(
            _ptr(out), C.c_uint64(out_capacity), _ptr(ooff), _ptr(_some(ores)), _ptr(_some(out_codecs)), _ptr(_some(tres)), _ptr(_some(frames)),
            C.c_uint64(frames_capacity), _ptr(foff), _ptr(_some(fres)), _ptr(_some(codecs)), _ptr(new_frames if nsel else None), C.c_uint64(new_capacity), _ptr(noff),
            _ptr(nres), _ptr(new_codecs if nsel else None), _ptr(_some(stage_results)), _ptr(soff), _ptr(_some(win)), SZ(n), C.c_uint(E), _ptr(sf), SZ(nseg), C.c_uint(L),
            _ptr(wf), SZ(nsel), _ptr(scratch), SZ(scratch.numel()), _stream()), what)
        for x in guards:
            x.check(what)
        return out, ooff, ores, tres, (out_codecs[:nseg] if out_codecs is not None else None)

    def _patch_window(self, what, transforms, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log, seg_first, n_segments, sel_first,
                      n_selected, stage_offsets, base, codec, codecs, new_codecs, block_size_id, capacity, frames_capacity, max_total_blocks, align_log, out, out_capacity,
                      out_offsets, out_results, out_codecs, tensor_results, stage, stage_capacity, stage_plane_offsets, stage_seg_offsets, stage_results, new_frames,
                      new_capacity, new_offsets, new_results, scratch, workspace, delta_op, stride_call=False, strides=None):
        """tensor_patch_window_dbatch (transforms None: one op for all), tensor_patch_window_each_dbatch (a transform per tensor) and, with
        stride_call, tensor_patch_window_each_stride_dbatch (`strides` as _strides takes them)"""
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        L = _seg_log(segment_log, min(block_size_id, 6))
        self._flat(frames, "frames")
        self._flat(src, "src")
        dev = frames.device
        if src.device != dev:
            raise ValueError("src is on %s, the frames on %s" % (src.device, dev))
        op = 0 if transforms is not None else _delta_op(delta_op)
        foff, _ = self._offsets(frame_offsets, dev, False)
        need_first = sel_first is None or max_total_blocks is None or stage_offsets is None
        soff, shost = self._offsets(src_offsets, dev, seg_first is None or need_first)
        n = soff.numel() - 1
        tr = None if transforms is None else _transforms(transforms, n, dev)
        held = _strides(strides, n, dev) if stride_call else None
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        frames_capacity = _room(self, frames, frames_capacity, "frames")
        win, whost = _windows(self, windows, dev, n)
        if seg_first is None:
            seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
        sf, nseg = _seg_first(self, seg_first, n_segments, dev, n * E)
        if foff.numel() < nseg + 1:
            raise ValueError("frame_offsets: one entry per segment (%d) and one more" % nseg)
        if frame_results is None:
            raise TypeError("frame_results: the results of the object's frames are needed")
        fres = _i64(self, frame_results, nseg, dev, "frame_results")
        if need_first:
            if whost is None:
                raise ValueError(what + ": windows on the device need sel_first, n_selected, stage_offsets and max_total_blocks")
            sizes = np.diff(shost.astype(np.int64)).clip(min=0)
            first, blocks = planes_window_first(self, sizes, whost, E, L, min(block_size_id, 6))
            sel_first = first if sel_first is None else sel_first
            max_total_blocks = blocks if max_total_blocks is None else max_total_blocks
            stage_offsets = planes_stage_offsets(self, sizes, whost, E, L) if stage_offsets is None else stage_offsets
        wf, nsel = _sel_first(self, sel_first, n_selected, dev, n * E)
        toff, thost = self._offsets(stage_offsets, dev, stage is None and stage_capacity is None)
        if toff.numel() != n + 1:
            raise ValueError("stage_offsets: one entry per tensor (%d) and one more" % n)
        if stage is None:
            stage_capacity = int(thost[-1]) if stage_capacity is None else int(stage_capacity)
            stage = torch.empty(max(stage_capacity, 1), dtype=torch.uint8, device=dev)
        else:
            stage_capacity = _room(self, stage, stage_capacity, "stage")
        mixed = codecs is not None
        choose = mixed and new_codecs is None
        if mixed:
            _u8(codecs, nseg, dev, "codecs")
            if choose and not isinstance(codec, AutoCodec):
                raise ValueError(what + ": an object with codecs needs an AutoCodec as `codec`, or new_codecs")
        elif new_codecs is not None or codec not in (0, 1):
            raise ValueError(what + ": an object without codecs takes codec 0 or 1 and no new_codecs")
        new_codecs, cgu = _codecs(self, new_codecs, nsel, dev) if mixed else (None, None)
        if new_frames is None:
            new_capacity = self.frame_packed_bound(stage_capacity, nsel, max_total_blocks, align_log) if new_capacity is None else int(new_capacity)
            new_frames = torch.empty(max(new_capacity, 1), dtype=torch.uint8, device=dev)
        else:
            new_capacity = _room(self, new_frames, new_capacity, "new_frames")
        out, out_capacity, out_codecs, guards = _splice_out(self, out, out_capacity, frames_capacity + new_capacity, codecs, out_codecs, nseg, dev)
        ooff = _i64(self, out_offsets, nseg + 1, dev, "out_offsets")
        ores = _i64(self, out_results, nseg, dev, "out_results")
        tres = _i64(self, tensor_results, n, dev, "tensor_results")
        spo = _i64(self, stage_plane_offsets, n * E + 1, dev, "stage_plane_offsets")
        sso = _i64(self, stage_seg_offsets, nsel + 1, dev, "stage_seg_offsets")
        sres = _i64(self, stage_results, n, dev, "stage_results")
        noff = _i64(self, new_offsets, nsel + 1, dev, "new_offsets")
        nres = _i64(self, new_results, nsel, dev, "new_results")
        if scratch is None:
            scratch = torch.empty(planes_splice_scratch_bound(self, n, E, nseg), dtype=torch.uint8, device=dev)
        workspace = _writer_workspace(self, workspace, nsel, max_total_blocks, block_size_id, codec, mixed, choose, dev)
        tol = codec.tolerance_permille if choose else 0
        front = (_ptr(out), C.c_uint64(out_capacity), _ptr(ooff), _ptr(_some(ores)), _ptr(_some(out_codecs)), _ptr(_some(tres)), _ptr(_some(frames)),
                 C.c_uint64(frames_capacity), _ptr(foff), _ptr(_some(fres)), _ptr(_some(codecs)), _ptr(_some(src)), _ptr(base))
        rest = (_ptr(soff), C.c_uint64(capacity), _ptr(_some(win)), SZ(n), C.c_uint(E), _ptr(sf), SZ(nseg), C.c_uint(L), _ptr(wf), SZ(nsel), _ptr(toff),
                C.c_uint64(stage_capacity), SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(0 if mixed else codec), _ptr(_some(new_codecs)),
                C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(tol), C.c_uint(align_log), _ptr(stage), _ptr(spo), _ptr(sso), _ptr(_some(sres)), _ptr(new_frames),
                C.c_uint64(new_capacity), _ptr(noff), _ptr(_some(nres)), _ptr(scratch), SZ(scratch.numel()), _ptr(workspace), SZ(workspace.numel()), _stream())
        if tr is None:
            _check(_call_base(self, "FSEHIP_tensor_patch_window_dbatch", op, 12, *front, *rest), what)
        elif stride_call:
            _check(self.lib.FSEHIP_tensor_patch_window_each_stride_dbatch(*front, VP(tr.data_ptr() or soff.data_ptr()), _ptr(held), *rest), what)
        else:
            _check(self.lib.FSEHIP_tensor_patch_window_each_dbatch(*front, VP(tr.data_ptr() or soff.data_ptr()), *rest), what)
        _check_codecs(cgu, nsel, what)
        for x in guards:
            x.check(what)
        return out, ooff, ores, tres, (out_codecs[:nseg] if out_codecs is not None else None)

    def tensor_patch_window_dbatch(self, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log, seg_first=None, n_segments=None,
                                   sel_first=None, n_selected=None, stage_offsets=None, base=None, codec=0, codecs=None, new_codecs=None, block_size_id=5,
                                   capacity=None, frames_capacity=None, max_total_blocks=None, align_log=0, out=None, out_capacity=None, out_offsets=None,
                                   out_results=None, out_codecs=None, tensor_results=None, stage=None, stage_capacity=None, stage_plane_offsets=None,
                                   stage_seg_offsets=None, stage_results=None, new_frames=None, new_capacity=None, new_offsets=None, new_results=None, scratch=None,
                                   workspace=None, delta_op=0):
        """-> (out, out_offsets, out_results, tensor_results, out_codecs): the object (frames, frame_offsets, frame_results, codecs) of
        tensor_compress_seg_dbatch brought up to date with `src`, the WHOLE current tensors in the layout src_offsets they were compressed in,
        which changed inside one window (a, b) of elements each.  The segments a >> segment_log .. (b - 1) >> segment_log of every plane are
        coded anew from src (XOR base, or zigzag(src - base) with delta_op 1), all other frames are the old ones byte for byte: planes_split_window_dbatch, planes_segments_dbatch
        over the stage, the packed writer, planes_splice_dbatch.  WHOLE SEGMENTS are replaced: inside a selected segment the bytes of src win
        outside the window too, elsewhere the old ones stay, so src must equal the object's content outside the windows (not checked).  For
        tensors that differ inside the windows only, the result is tensor_compress_seg_dbatch of src, byte for byte.
        codecs None: `codec` 0 / 1 for every new frame.  codecs the object's (one per segment): `codec` an AutoCodec -- the new frames' codecs
        are chosen by size -- or new_codecs given (one per selected frame).  align_log: what the object was written with.  tensor_results
        and capacity as planes_splice_dbatch; out_capacity None: frames_capacity + frame_packed_bound of the staged bytes.  sel_first,
        stage_offsets or max_total_blocks None: planes_window_first / planes_stage_offsets (src_offsets and windows then on the host).  The
        stage, its offsets and results, the new frames, the scratch and the writer's workspace for n_selected frames are scratch; with
        everything given and on the device the call is launches only."""
        return _patch_window(self, "tensor_patch_window_dbatch", None, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log,
                             seg_first, n_segments, sel_first, n_selected, stage_offsets, base, codec, codecs, new_codecs, block_size_id, capacity, frames_capacity,
                             max_total_blocks, align_log, out, out_capacity, out_offsets, out_results, out_codecs, tensor_results, stage, stage_capacity, stage_plane_offsets,
                             stage_seg_offsets, stage_results, new_frames, new_capacity, new_offsets, new_results, scratch, workspace, delta_op)

    def patch_tensor_windows(self, obj, tensors, windows, base=None):
        """-> a NEW CompressedTensors: `obj` (of compress_tensors_segmented) brought up to date with `tensors`, the WHOLE current CUDA tensors --
        one per tensor of the object, of its dtype, shape and device -- which changed inside the elements [start, stop) of the flattened tensor
        that `windows` names: one entry per tensor, None (nothing changed) or (start, stop) with 0 <= start <= stop <= numel.  Only the segment
        frames that hold a window are coded again (tensor_patch_window_dbatch); every other frame is copied as it is.  The patch works on
        WHOLE SEGMENTS of 1 << segment_log bytes per plane: inside a segment that holds part of a window all bytes come from `tensors`,
        elsewhere the old ones stay -- so `tensors` must equal the object's content outside the windows, which is not checked.  Where they do,
        the result is what compress_tensors_segmented(tensors) gives, byte for byte.  `obj` is not changed.  The new object has the same
        segment_log, block_size_id, delta, codec and seg_first; an object written with an AutoCodec has the codecs of the new frames chosen
        anew.  base: for an object with `delta` set, the whole base tensors as compress_tensors takes them.  ValueError / TypeError before any
        launch: an object that is not segmented, a wrong number of tensors or windows, a tensor of another dtype, shape or device, a window
        that is not one, a base / delta mismatch.  `base_digests` of the object are not checked here and are carried over to the new one: the
        patch is a delta against the same base."""
        seg_log = getattr(obj, "segment_log", None)
        if seg_log is None:
            raise ValueError("patch_tensor_windows: the object is not segmented (compress_tensors_segmented writes those)")
        _not_sparse(obj, "patch_tensor_windows")
        base, op = _read_base(obj, base, "patch_tensor_windows")
        tensors, windows = list(tensors), list(windows)
        if len(tensors) != len(obj.dtypes) or len(windows) != len(obj.dtypes):
            raise ValueError("patch_tensor_windows: %d tensors and %d windows for %d tensors" % (len(tensors), len(windows), len(obj.dtypes)))
        for k, (t, dt, sh) in enumerate(zip(tensors, obj.dtypes, obj.shapes)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != obj.device or t.dtype != dt:
                raise TypeError("patch_tensor_windows: tensor %d: a CUDA tensor of %s on %s is needed" % (k, dt, obj.device))
            if tuple(t.shape) != tuple(sh):
                raise ValueError("patch_tensor_windows: tensor %d has shape %s, the object's has %s" % (k, tuple(t.shape), tuple(sh)))
        wins = []
        for k, (w, sh) in enumerate(zip(windows, obj.shapes)):
            numel = int(np.prod(sh, dtype=np.int64))
            if w is not None and (not isinstance(w, (tuple, list)) or len(w) != 2 or any(not isinstance(x, numbers.Integral) or isinstance(x, bool) for x in w)
                                  or not 0 <= w[0] <= w[1] <= numel):
                raise ValueError("patch_tensor_windows: window %d is %r, None or (start, stop) with 0 <= start <= stop <= %d is needed" % (k, w, numel))
            wins.append((0, 0) if w is None else (int(w[0]), int(w[1])))
        braw = None if base is None else _bases(base, obj.dtypes, obj.shapes, obj.device)
        auto = isinstance(obj.codec, AutoCodec)
        groups = []
        for g in obj.groups:
            E, sizes, idx = g["elem_bytes"], g["sizes"], g["index"]
            gw = [wins[i] for i in idx]
            new = dict(g)
            if any(b > a for a, b in gw):
                raw = [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx]
                offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
                src = torch.cat(raw)
                bsrc = None if braw is None else torch.cat([braw[i] for i in idx])
                first, blocks = self.planes_window_first(sizes, gw, E, seg_log, obj.block_size_id)
                toff = self.planes_stage_offsets(sizes, gw, E, seg_log)
                cap = int(g["frames"].numel()) + self.frame_packed_bound(int(toff[-1]), int(first[-1]), blocks, 0)
                out, ooff, ores, tres, ocod = self.tensor_patch_window_dbatch(
                    g["frames"], g["frame_offsets"], g["frame_results"], src, offs, gw, E, seg_log, g["seg_first"], sel_first=first, stage_offsets=toff, base=bsrc,
                    codec=obj.codec if auto or "codecs" not in g else 0, codecs=g.get("codecs"), block_size_id=obj.block_size_id, max_total_blocks=blocks,
                    out_capacity=cap, delta_op=op)
                got = torch.cat([ooff[-1:], tres]).cpu().tolist()
                if got[1:] != sizes or got[0] > cap:
                    raise RuntimeError("patch_tensor_windows: element size %d, results %s for tensors of %s bytes" % (E, got[1:9], sizes[:8]))
                new.update(frames=out[:got[0]].clone(), frame_offsets=ooff, frame_results=ores, tensor_results=tres)
                if ocod is not None:
                    new["codecs"] = ocod.clone()
            else:
                new.update(frames=g["frames"].clone(), frame_offsets=g["frame_offsets"].clone(), frame_results=g["frame_results"].clone(),
                           tensor_results=g["tensor_results"].clone())
                if "codecs" in g:
                    new["codecs"] = g["codecs"].clone()
            groups.append(new)
        return _segmented(CompressedTensors(groups, list(obj.dtypes), list(obj.shapes), obj.device, obj.codec, obj.block_size_id, obj.delta), seg_log,
                          getattr(obj, "delta_op", "xor"), None, getattr(obj, "base_digests", None))

    # ---- patching tensors with a transform per tensor (fsehip.h, the section of that name): the write side of the windows for frames of
    # tensor_compress_seg_each_dbatch and tensor_compress_seg_pred_dbatch
    def planes_split_window_each_dbatch(self, src, src_offsets, windows, elem_bytes, segment_log, transforms, stage_offsets=None, base=None, capacity=None, stage=None,
                                        stage_capacity=None, plane_offsets=None, results=None):
        """planes_split_window_dbatch with tensor i staged as transforms[i] says (names, ids or a CUDA uint8 tensor, as planes_split_each_dbatch
        takes them): for "plain", "xor" and "sub" byte for byte what planes_split_window_dbatch stages (no base, delta_op 0, delta_op 1), for
        "pred" segments k0 .. k1 of the planes planes_split_pred_dbatch writes for the whole tensor -- a segment starts on a run of 1024
        elements, so nothing in front of the staged bytes is read.  base: laid out as src, read for xor and sub tensors only.  results -1 and
        all plane offsets the tensor's stage offset, nothing of it read or written, also for a byte that is none of the four and for xor /
        sub without a base."""
        return _split_window(self, "planes_split_window_each_dbatch", transforms, src, src_offsets, windows, elem_bytes, segment_log, stage_offsets, base, capacity, stage,
                             stage_capacity, plane_offsets, results, 0)

    def tensor_patch_window_each_dbatch(self, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log, transforms, seg_first=None,
                                        n_segments=None, sel_first=None, n_selected=None, stage_offsets=None, base=None, codec=0, codecs=None, new_codecs=None,
                                        block_size_id=5, capacity=None, frames_capacity=None, max_total_blocks=None, align_log=0, out=None, out_capacity=None,
                                        out_offsets=None, out_results=None, out_codecs=None, tensor_results=None, stage=None, stage_capacity=None,
                                        stage_plane_offsets=None, stage_seg_offsets=None, stage_results=None, new_frames=None, new_capacity=None, new_offsets=None,
                                        new_results=None, scratch=None, workspace=None):
        """tensor_patch_window_dbatch for an object that tensor_compress_seg_each_dbatch wrote with these transforms (names, ids or a CUDA uint8
        tensor; all "pred": an object of tensor_compress_seg_pred_dbatch): planes_split_window_each_dbatch, then the segments kernel, the packed
        writer and the splice as they are.  Every other argument, the scratch, the workspace and the results are those of
        tensor_patch_window_dbatch.  For tensors that differ inside the windows only, the result is tensor_compress_seg_each_dbatch of src with
        the same transforms given, byte for byte.  The transforms are GIVEN: the patch never chooses again.  base is read for xor and sub
        tensors only; without one those are refused alone (-1) and keep all their old frames, like a tensor whose byte is none of the four."""
        return _patch_window(self, "tensor_patch_window_each_dbatch", transforms, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log,
                             seg_first, n_segments, sel_first, n_selected, stage_offsets, base, codec, codecs, new_codecs, block_size_id, capacity, frames_capacity,
                             max_total_blocks, align_log, out, out_capacity, out_offsets, out_results, out_codecs, tensor_results, stage, stage_capacity, stage_plane_offsets,
                             stage_seg_offsets, stage_results, new_frames, new_capacity, new_offsets, new_results, scratch, workspace, 0)

    def patch_tensor_windows_each(self, obj, tensors, windows, base=None):
        """patch_tensor_windows for ANY segmented object that is not sparse, with the same contract -- the WHOLE current CUDA tensors, one window
        (start, stop) or None per tensor, whole segments replaced, a NEW object that shares nothing with `obj`, which is not changed; only the
        segment frames that hold a window are coded again (tensor_patch_window_each_dbatch):
          an object of compress_tensors_each(..., segment_log=...), also reopened from an archive: obj.transforms, per tensor, GIVEN -- the
            patch never chooses a transform again; base (the base of the whole list) iff one of them is "xor" or "sub";
          an object written with PredictedPlanes (predictor "prev"): every tensor "pred", no base;
          a plain or a delta object of compress_tensors_segmented: every tensor "plain", or "xor" / "sub" by the object's delta_op with its base.
        Where `tensors` equal the object's content outside the windows the result is what the compress call that wrote `obj` gives for
        `tensors` (with obj.transforms given), byte for byte.  A window of a "pred" tensor may start anywhere: a segment starts on a run.
        The new object carries transforms or predictor, segment_log, block_size_id, codec, delta, delta_op, base_digests and seg_first over;
        with an AutoCodec the codecs of the new frames are chosen anew.  ValueError / TypeError before any launch: no segment_log; a sparse
        object; a wrong number of tensors or windows; a tensor of another dtype, shape or device; a window that is not one; transforms that
        are not names out of EST_NAMES, or together with a predictor; a predictor other than "prev"; "xor" / "sub" tensors without a base;
        a base for an object that holds neither."""
        return _patch_windows_each(self, "patch_tensor_windows_each", obj, tensors, windows, base, False)

    def patch_tensor_windows_each_stride(self, obj, tensors, windows, base=None):
        """patch_tensor_windows_each for objects that hold a stride above 1 as well, with the same contract and the same refusals but that one
        (tensor_patch_window_each_stride_dbatch).  It takes everything patch_tensor_windows_each takes -- the stride is then 1 everywhere -- and
          an object of compress_tensors_each(..., strides=..., segment_log=...): obj.strides, one integer 1 .. 8 per tensor, GIVEN beside
            obj.transforms -- the patch chooses neither again;
          a segmented object written with PredictedPlanes(codec, stride=S) (predictor "prev<S>"): every tensor "pred" at stride S;
          all of these reopened from an archive or a file.
        A staged segment starts a run of 1024 elements for every one of the S chains, so a window may start anywhere and no element in front
        of a segment is read.  Where `tensors` equal the object's content outside the windows the result is what the compress call that
        wrote `obj` gives for `tensors` with obj.transforms and obj.strides given, byte for byte.  The new object carries strides or predictor
        over, together with what patch_tensor_windows_each carries.  ValueError / TypeError before any launch: those of
        patch_tensor_windows_each; strides that are not one integer 1 .. 8 per tensor; a predictor that predictor_stride does not know."""
        return _patch_windows_each(self, "patch_tensor_windows_each_stride", obj, tensors, windows, base, True)

    def _patch_windows_each(self, what, obj, tensors, windows, base, strided):
        """the body of patch_tensor_windows_each (strided False: an object with a stride above 1 is refused) and of
        patch_tensor_windows_each_stride"""
        seg_log = getattr(obj, "segment_log", None)
        if seg_log is None:
            raise ValueError(what + ": the object is not segmented (compress_tensors_each and compress_tensors_segmented write those with a segment_log)")
        if getattr(obj, "sparse_permille", None) is not None:
            raise ValueError(what + ": the object holds sparse planes (SparsePlanes); patches of those are not supported")
        if not strided and any(st != 1 for st in (getattr(obj, "strides", None) or ())):
            raise ValueError(what + ": the object holds a stride above 1 (compress_tensors_each with strides); patches of those are not supported here, "
                             "patch_tensor_windows_each_stride takes them")
        strides = _obj_strides(obj, what) if strided else None
        n = len(obj.dtypes)
        names, predictor = getattr(obj, "transforms", None), getattr(obj, "predictor", None)
        if names is not None:
            names = list(names)
            if len(names) != n or any(not isinstance(t, str) or t not in EST_NAMES for t in names):
                raise ValueError("%s: transforms %r; one name per tensor (%d) out of %r is needed" % (what, names[:8], n, EST_NAMES))
            if predictor is not None:
                raise ValueError(what + ": a predictor does not go with a transform per tensor")
            if isinstance(base, DeltaBase):
                base = base.tensors
            if any(t in ("xor", "sub") for t in names) != (base is not None):
                raise ValueError(what + ": the object holds \"xor\" or \"sub\" tensors and needs its base" if base is None else
                                 what + ": the object holds no \"xor\" or \"sub\" tensor, a base does not belong to it")
        elif predictor is not None:
            if strided:
                strides = [predictor_stride(predictor, what)] * n
            elif predictor != "prev":
                raise ValueError("%s: predictor %r; only \"prev\" is known (patch_tensor_windows_each_stride takes \"prev2\" .. \"prev%d\")" %
                                 (what, predictor, PRED_MAX_STRIDE))
            if base is not None:
                raise ValueError(what + ": the object holds predicted planes, a base does not belong to it")
            names = ["pred"] * n
        else:
            base, op = _read_base(obj, base, what)
            names = [("plain" if base is None else "sub" if op else "xor")] * n
        tensors = list(tensors)
        if len(tensors) != n:
            raise ValueError("%s: %d tensors for %d tensors" % (what, len(tensors), n))
        wins = [w or (0, 0) for w in _window_list(what, obj, windows)]
        for k, (t, dt, sh) in enumerate(zip(tensors, obj.dtypes, obj.shapes)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != obj.device or t.dtype != dt:
                raise TypeError("%s: tensor %d: a CUDA tensor of %s on %s is needed" % (what, k, dt, obj.device))
            if tuple(t.shape) != tuple(sh):
                raise ValueError("%s: tensor %d has shape %s, the object's has %s" % (what, k, tuple(t.shape), tuple(sh)))
        braw = None if base is None else _bases(base, obj.dtypes, obj.shapes, obj.device)
        inner = obj.codec.codec if isinstance(obj.codec, PredictedPlanes) else obj.codec
        auto = isinstance(inner, AutoCodec)
        groups = []
        for g in obj.groups:
            E, sizes, idx = g["elem_bytes"], g["sizes"], g["index"]
            gw = [wins[i] for i in idx]
            new = dict(g)
            if any(b > a for a, b in gw):
                raw = [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx]
                offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
                src = torch.cat(raw)
                bsrc = None if braw is None else torch.cat([braw[i] for i in idx])
                first, blocks = self.planes_window_first(sizes, gw, E, seg_log, obj.block_size_id)
                toff = self.planes_stage_offsets(sizes, gw, E, seg_log)
                cap = int(g["frames"].numel()) + self.frame_packed_bound(int(toff[-1]), int(first[-1]), blocks, 0)
                more = dict(sel_first=first, stage_offsets=toff, base=bsrc, codec=inner if auto or "codecs" not in g else 0, codecs=g.get("codecs"),
                            block_size_id=obj.block_size_id, max_total_blocks=blocks, out_capacity=cap)
                if strided:
                    out, ooff, ores, tres, ocod = self.tensor_patch_window_each_stride_dbatch(
                        g["frames"], g["frame_offsets"], g["frame_results"], src, offs, gw, E, seg_log, [names[i] for i in idx],
                        None if strides is None else [strides[i] for i in idx], g["seg_first"], **more)
                else:
                    out, ooff, ores, tres, ocod = tensor_patch_window_each_dbatch(
                        self, g["frames"], g["frame_offsets"], g["frame_results"], src, offs, gw, E, seg_log, [names[i] for i in idx], g["seg_first"], **more)
                got = torch.cat([ooff[-1:], tres]).cpu().tolist()
                if got[1:] != sizes or got[0] > cap:
                    raise RuntimeError("%s: element size %d, results %s for tensors of %s bytes" % (what, E, got[1:9], sizes[:8]))
                new.update(frames=out[:got[0]].clone(), frame_offsets=ooff, frame_results=ores, tensor_results=tres)
                if ocod is not None:
                    new["codecs"] = ocod.clone()
            else:
                new.update(frames=g["frames"].clone(), frame_offsets=g["frame_offsets"].clone(), frame_results=g["frame_results"].clone(),
                           tensor_results=g["tensor_results"].clone())
                if "codecs" in g:
                    new["codecs"] = g["codecs"].clone()
            groups.append(new)
        got = _segmented(CompressedTensors(groups, list(obj.dtypes), list(obj.shapes), obj.device, obj.codec, obj.block_size_id, obj.delta), seg_log,
                         getattr(obj, "delta_op", "xor"), None, getattr(obj, "base_digests", None), predictor)
        if getattr(obj, "transforms", None) is not None:
            got.transforms = list(names)
        if getattr(obj, "strides", None) is not None:
            got.strides = [int(st) for st in obj.strides]
        return got

    for f in (planes_stage_offsets, planes_split_window_dbatch, planes_splice_scratch_bound, planes_splice_dbatch, tensor_patch_window_dbatch, patch_tensor_windows,
              planes_split_window_each_dbatch, tensor_patch_window_each_dbatch, patch_tensor_windows_each, patch_tensor_windows_each_stride):
        setattr(FseHip, f.__name__, f)

    # ---- sparse planes (csrc/planes_sparse.hip; fsehip.h "sparse planes"): a unit of n bytes as a zero mask of ceil(n / 8) bytes and its
    # non-zero bytes where that is shorter and the unit sparse enough, ahead of the frame writers and behind the frame reader
    def _permille(permille):
        if not isinstance(permille, numbers.Integral) or isinstance(permille, bool) or not 0 <= permille <= 1000:
            raise ValueError("sparse permille %r: 0 .. 1000" % (permille,))
        return int(permille)

    def sparse_workspace_bound(self, capacity, n_units):
        """the workspace of sparse_pack_dbatch / sparse_expand_dbatch for n_units units inside `capacity` bytes.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_sparse_workspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_sparse_workspaceBound(C.c_uint64(int(capacity)), SZ(int(n_units))))
        if r >= (1 << 62):
            raise ValueError("sparse_workspace_bound(%r, %r)" % (capacity, n_units))
        return r

    def _sparse_ws(self, workspace, capacity, n_units, rest, device):
        """the caller's workspace, or one of sparse_workspace_bound + `rest` (the writer's or the reader's need) bytes"""
        if workspace is not None:
            return workspace
        return torch.empty(sparse_workspace_bound(self, capacity, n_units) + max(int(rest), 1), dtype=torch.uint8, device=device)

    def sparse_pack_dbatch(self, units, unit_offsets, permille=500, capacity=None, contents=None, content_offsets=None, workspace=None):
        """-> (contents, content_offsets): unit u = units[unit_offsets[u] : unit_offsets[u+1]] becomes content u =
        contents[content_offsets[u] : content_offsets[u+1]] -- its zero mask and its non-zero bytes if at most permille / 1000 of its bytes
        are non-zero and that is shorter, else the unit itself.  content_offsets (n + 1) are directly the src_offsets of the packed writers.
        `capacity` (default: units' size) is the size of both buffers; `contents` must not overlap `units`."""
        self._flat(units, "units")
        uoff, _ = self._offsets(unit_offsets, units.device, False)
        n = uoff.numel() - 1
        capacity = _room(self, units, capacity, "units")
        g = None
        if contents is None:
            contents, g = self._dst(1, capacity, units.device)
            contents = contents[0]
        elif _room(self, contents, None, "contents") < capacity:
            raise ValueError("contents holds %d bytes, the capacity is %d" % (contents.numel(), capacity))
        coff = _i64(self, content_offsets, n + 1, units.device, "content_offsets")
        workspace = _sparse_ws(self, workspace, capacity, n, 0, units.device)
        _check(self.lib.FSEHIP_sparse_pack_dbatch(_ptr(contents), _ptr(coff), _ptr(units), _ptr(uoff), SZ(n), C.c_uint64(capacity), C.c_uint(_permille(permille)),
                                                  _ptr(workspace), SZ(workspace.numel()), _stream()), "sparse_pack_dbatch")
        if g is not None:
            g.check("sparse_pack_dbatch")
        return contents, coff

    def sparse_expand_dbatch(self, contents, content_offsets, content_results, unit_offsets, units=None, capacity=None, contents_capacity=None, results=None,
                             workspace=None):
        """-> (units, results): the inverse.  content u = contents[content_offsets[u] : + content_results[u]] (what frame_decompress_packed_dbatch
        leaves in dst_offsets / results: negative results are errors and pass through), unit u is rebuilt at units[unit_offsets[u]:], its size
        EXACTLY unit_offsets[u+1] - unit_offsets[u].  results[u] = that size, the reader's error, or -4 (corruption_detected: a content longer
        than its unit or shorter than its mask, a popcount that is not the number of values, a set padding bit, a zero among the values);
        such a unit is not written."""
        self._flat(contents, "contents")
        uoff, uhost = self._offsets(unit_offsets, contents.device, units is None)
        n = uoff.numel() - 1
        coff = _i64(self, content_offsets, n + 1, contents.device, "content_offsets")
        cres = _i64(self, content_results, n, contents.device, "content_results")
        contents_capacity = _room(self, contents, contents_capacity, "contents")
        units, capacity, g = _dst_room(self, units, capacity, uhost, contents.device)
        res = _i64(self, results, n, contents.device, "results")
        workspace = _sparse_ws(self, workspace, capacity, n, 0, contents.device)
        _check(self.lib.FSEHIP_sparse_expand_dbatch(_ptr(units), _ptr(res), _ptr(uoff), SZ(n), C.c_uint64(capacity), _ptr(contents), C.c_uint64(contents_capacity),
                                                    _ptr(coff), _ptr(cres), _ptr(workspace), SZ(workspace.numel()), _stream()), "sparse_expand_dbatch")
        if g is not None:
            g.check("sparse_expand_dbatch")
        return units, res

    def _compress_sparse(self, what, src, src_offsets, elem_bytes, permille, segment_log, seg_first, n_segments, base, codec, codecs, block_size_id, capacity, dst,
                         dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, seg_offsets, contents,
                         content_offsets, workspace, delta_op):
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        permille = _permille(permille)
        seg = segment_log is not None
        L = _seg_log(segment_log, min(block_size_id, 6)) if seg else 0
        self._flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, (seg and seg_first is None) or max_total_blocks is None or (dst is None and dst_capacity is None))
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        op = _delta_op(delta_op)
        _base(self, base, src, capacity, "src")
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, src.device, n * E)
        else:
            sf, nf = None, n * E
        mixed = codecs is not None or isinstance(codec, AutoCodec)
        choose = mixed and codecs is None
        codecs, cgu = _codecs(self, codecs, nf, src.device) if mixed else (None, None)
        max_total_blocks, dst, dst_capacity, g = _frames_room(self, shost, n, E, nf, block_size_id, max_total_blocks, dst, dst_capacity, align_log, src.device)
        planes = _split_room(self, planes, src, capacity, E > 1 or base is not None)
        foff = _i64(self, frame_offsets, nf + 1, src.device, "frame_offsets")
        fres = _i64(self, frame_results, nf, src.device, "frame_results")
        tres = _i64(self, tensor_results, n, src.device, "tensor_results")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        so = _i64(self, seg_offsets, nf + 1, src.device, "seg_offsets") if seg else None
        cg = None
        if contents is None:
            contents, cg = self._dst(1, capacity, src.device)
            contents = contents[0]
        elif _room(self, contents, None, "contents") < capacity:
            raise ValueError("contents holds %d bytes, the capacity is %d" % (contents.numel(), capacity))
        coff = _i64(self, content_offsets, nf + 1, src.device, "content_offsets")
        if workspace is None:
            workspace = _sparse_ws(self, None, capacity, nf, _writer_need(self, nf, max_total_blocks, block_size_id, codec, mixed, choose), src.device)
        tol = codec.tolerance_permille if choose and isinstance(codec, AutoCodec) else 0
        head = (_ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src), _ptr(base), C.c_uint(op), _ptr(soff), SZ(n), C.c_uint(E),
                C.c_uint64(capacity))
        writer = (SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(0 if mixed else codec),
                  _ptr((codecs if codecs.numel() else codecs.new_zeros(1)) if mixed else None), C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(tol),
                  C.c_uint(align_log), C.c_uint(permille), _ptr(planes), _ptr(poff))
        tail = (_ptr(contents), _ptr(coff), _ptr(workspace), SZ(workspace.numel()), _stream())
        if seg:
            _check(self.lib.FSEHIP_tensor_compress_seg_sparse_dbatch(*head, _ptr(sf), SZ(nf), C.c_uint(L), *writer, _ptr(so), *tail), what)
        else:
            _check(self.lib.FSEHIP_tensor_compress_sparse_dbatch(*head, *writer, *tail), what)
        _check_codecs(cgu, nf, what)
        for x in (g, cg):
            if x is not None:
                x.check(what)
        return dst, foff, fres, tres, (codecs[:nf] if mixed else None)

    def tensor_compress_sparse_dbatch(self, src, src_offsets, elem_bytes, permille=500, base=None, codec=0, codecs=None, block_size_id=5, capacity=None, dst=None,
                                      dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None,
                                      plane_offsets=None, contents=None, content_offsets=None, workspace=None, delta_op=0):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs): the split (against `base` if one is given, by delta_op),
        sparse_pack_dbatch over the planes at `permille`, then the packed writer over the contents -- frame i*E+p is the .fse frame of the
        content of plane p of tensor i.  codec / codecs as tensor_compress_seg_dbatch takes them (0 / 1, an AutoCodec, or a codec per frame
        given).  planes, plane_offsets (n*E+1), contents (`capacity` bytes) and content_offsets (n*E+1) are scratch; the workspace is
        sparse_workspace_bound(capacity, n*E) followed by the (mixed) writer's.  With everything given the call is launches only."""
        return _compress_sparse(self, "tensor_compress_sparse_dbatch", src, src_offsets, elem_bytes, permille, None, None, None, base, codec, codecs, block_size_id,
                                capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, None,
                                contents, content_offsets, workspace, delta_op)

    def tensor_compress_seg_sparse_dbatch(self, src, src_offsets, elem_bytes, segment_log, permille=500, seg_first=None, n_segments=None, base=None, codec=0,
                                          codecs=None, block_size_id=5, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0,
                                          frame_offsets=None, frame_results=None, tensor_results=None, planes=None, plane_offsets=None, seg_offsets=None, contents=None,
                                          content_offsets=None, workspace=None, delta_op=0):
        """tensor_compress_seg_dbatch with sparse_pack_dbatch between the segments kernel and the writer: a unit is a SEGMENT of a plane, every
        segment decides for itself.  contents and content_offsets (n_segments+1) are scratch beside the segmented call's; the workspace is
        sparse_workspace_bound(capacity, n_segments) followed by the (mixed) writer's for n_segments frames."""
        return _compress_sparse(self, "tensor_compress_seg_sparse_dbatch", src, src_offsets, elem_bytes, permille, segment_log, seg_first, n_segments, base, codec,
                                codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes,
                                plane_offsets, seg_offsets, contents, content_offsets, workspace, delta_op)

    def _decompress_sparse(self, what, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first, n_segments, base, dst, dst_capacity, max_total_blocks,
                           contents, contents_capacity, content_offsets, content_results, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes,
                           workspace, results, delta_op):
        E = _elem(elem_bytes)
        seg = segment_log is not None
        L = _seg_log(segment_log) if seg else 0
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None or planes is None or contents is None or (seg and seg_first is None))
        n = doff.numel() - 1
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(dhost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, frames.device, n * E)
        else:
            sf, nf = None, n * E
        if foff.numel() != nf + 1:
            raise ValueError("frame_offsets: one entry per frame (%d) and one more" % nf)
        if max_total_blocks is None:
            _, bfirst = self.frame_plan_dbatch(frames, foff, None, 0)
            max_total_blocks = int(bfirst[nf].item())
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, None if planes is not None else int(dhost[-1]), frames.device)
        contents, contents_capacity = _planes_room(self, contents, contents_capacity, None if contents is not None else int(dhost[-1]), frames.device)
        coff = _i64(self, content_offsets, nf + 1, frames.device, "content_offsets")
        cres = _i64(self, content_results, nf, frames.device, "content_results")
        poff = _i64(self, plane_offsets, n * E + 1, frames.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, frames.device, "plane_sizes")
        res = _i64(self, results, n, frames.device, "results")
        if workspace is None:
            workspace = _sparse_ws(self, None, min(dst_capacity, planes_capacity), nf, _reader_need(self, nf, max_total_blocks), frames.device)
        op = _delta_op(delta_op)
        _base(self, base, frames, dst_capacity, "dst")
        head = (_ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(base), C.c_uint(op), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), C.c_uint(E))
        mid = (SZ(max_total_blocks), _ptr(contents), C.c_uint64(contents_capacity), _ptr(coff), _ptr(cres), _ptr(planes), C.c_uint64(planes_capacity))
        tail = (_ptr(poff), _ptr(psz), _ptr(workspace), SZ(workspace.numel()), _stream())
        if seg:
            so = _i64(self, seg_offsets, nf + 1, frames.device, "seg_offsets")
            sres = _i64(self, seg_results, nf, frames.device, "seg_results")
            _check(self.lib.FSEHIP_tensor_decompress_seg_sparse_dbatch(*head, _ptr(sf), SZ(nf), C.c_uint(L), *mid, _ptr(so), _ptr(sres), *tail), what)
        else:
            _check(self.lib.FSEHIP_tensor_decompress_sparse_dbatch(*head, *mid, *tail), what)
        if g is not None:
            g.check(what)
        return dst, res

    def tensor_decompress_sparse_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, base=None, dst=None, dst_capacity=None, max_total_blocks=None,
                                        contents=None, contents_capacity=None, content_offsets=None, content_results=None, planes=None, planes_capacity=None,
                                        plane_offsets=None, plane_results=None, workspace=None, results=None, delta_op=0):
        """-> (dst, results): the packed reader into `contents`, sparse_expand_dbatch into `planes`, then the merge (against `base` if one is
        given, by delta_op; dst may be `base` itself) into the slots dst_offsets.  A tensor's size is EXACTLY its slot -- stricter than
        tensor_decompress_dbatch: the reader has to know every plane's size to tell a sparse content from a dense one.  It reads frames of
        tensor_compress_dbatch and its delta and mixed forms as well (all contents dense).  results[i] = the tensor's size, or the error
        of the first of its frames or contents that fails; such a tensor's slot is not written.  The workspace is
        sparse_workspace_bound(min(dst_capacity, planes_capacity), n*E) followed by the packed reader's."""
        return _decompress_sparse(self, "tensor_decompress_sparse_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, None, None, None, base, dst, dst_capacity,
                                  max_total_blocks, contents, contents_capacity, content_offsets, content_results, planes, planes_capacity, None, None, plane_offsets,
                                  plane_results, workspace, results, delta_op)

    def tensor_decompress_seg_sparse_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None, base=None, dst=None,
                                            dst_capacity=None, max_total_blocks=None, contents=None, contents_capacity=None, content_offsets=None, content_results=None,
                                            planes=None, planes_capacity=None, seg_offsets=None, seg_results=None, plane_offsets=None, plane_sizes=None, workspace=None,
                                            results=None, delta_op=0):
        """tensor_decompress_seg_dbatch for frames of tensor_compress_seg_sparse_dbatch: the packed reader into `contents`, sparse_expand_dbatch
        over the segment layout of the slots into `planes`, the fold, the merge.  A tensor's size is exactly its slot."""
        return _decompress_sparse(self, "tensor_decompress_seg_sparse_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first, n_segments, base,
                                  dst, dst_capacity, max_total_blocks, contents, contents_capacity, content_offsets, content_results, planes, planes_capacity, seg_offsets,
                                  seg_results, plane_offsets, plane_sizes, workspace, results, delta_op)

    for f in (sparse_workspace_bound, sparse_pack_dbatch, sparse_expand_dbatch, tensor_compress_sparse_dbatch, tensor_decompress_sparse_dbatch,
              tensor_compress_seg_sparse_dbatch, tensor_decompress_seg_sparse_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- predicted planes (csrc/planes_pred.hip; fsehip.h "predicted planes"): the planes of zigzag(element - the element in front of it)
    # in runs of 1024 elements, the difference fused into the split and the run sums into the merge
    _NO_STRIDE = object()                                    # the _pred_ exports take no stride; the _pred_stride_ ones take 1 .. 8

    def _stride(stride, what):
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= PRED_MAX_STRIDE:
            raise ValueError("%s: stride %r, an integer 1 .. %d is needed" % (what, stride, PRED_MAX_STRIDE))
        return (C.c_uint(int(stride)),)

    def planes_split_pred_dbatch(self, src, src_offsets, elem_bytes, capacity=None, planes=None, plane_offsets=None, results=None, _stride_arg=_NO_STRIDE):
        """planes_split_dbatch of the neighbour differences: the same layout, offsets and results.  For every elem_bytes, 1 included, `planes`
        is a buffer of its own and is written; src is only read."""
        what = "planes_split_pred_dbatch" if _stride_arg is _NO_STRIDE else "planes_split_pred_stride_dbatch"
        st = () if _stride_arg is _NO_STRIDE else _stride(_stride_arg, what)      # (the _pred_ export takes none)
        E = _elem(elem_bytes)
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        g = None
        if planes is None:
            planes, g = self._dst(1, src.numel(), src.device)
            planes = planes[0]
        elif _room(self, planes, None, "planes") < capacity:
            raise ValueError("planes holds %d bytes, the capacity is %d" % (planes.numel(), capacity))
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        res = _i64(self, results, n, src.device, "results")
        call = self.lib.FSEHIP_planes_split_pred_dbatch if _stride_arg is _NO_STRIDE else self.lib.FSEHIP_planes_split_pred_stride_dbatch
        _check(call(_ptr(planes), _ptr(poff), _ptr(res), _ptr(src), _ptr(soff), SZ(n), C.c_uint(E), C.c_uint64(capacity), *st, _stream()), what)
        if g is not None:
            g.check(what)
        return planes, poff, res

    def planes_merge_pred_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, dst=None, capacity=None, results=None, _stride_arg=_NO_STRIDE):
        """planes_merge_dbatch, every run of a rebuilt tensor summed back: the inverse of planes_split_pred_dbatch, with the plain merge's
        results and rules.  dst must not overlap planes."""
        what = "planes_merge_pred_dbatch" if _stride_arg is _NO_STRIDE else "planes_merge_pred_stride_dbatch"
        st = () if _stride_arg is _NO_STRIDE else _stride(_stride_arg, what)      # (the _pred_ export takes none)
        E = _elem(elem_bytes)
        self._flat(planes, "planes")
        doff, dhost = self._offsets(dst_offsets, planes.device, dst is None)
        n = doff.numel() - 1
        poff = _i64(self, plane_offsets, n * E, planes.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, planes.device, "plane_sizes")
        dst, capacity, g = _dst_room(self, dst, capacity, dhost, planes.device)
        res = _i64(self, results, n, planes.device, "results")
        call = self.lib.FSEHIP_planes_merge_pred_dbatch if _stride_arg is _NO_STRIDE else self.lib.FSEHIP_planes_merge_pred_stride_dbatch
        _check(call(_ptr(dst), _ptr(doff), _ptr(res), _ptr(planes), _ptr(poff), _ptr(psz), SZ(n), C.c_uint(E), C.c_uint64(capacity), *st, _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    def _compress_pred(self, what, src, src_offsets, elem_bytes, segment_log, seg_first, n_segments, codec, codecs, block_size_id, capacity, dst, dst_capacity,
                       max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, seg_offsets, workspace, stride=_NO_STRIDE):
        st = () if stride is _NO_STRIDE else _stride(stride, what)               # (the _pred_ exports take none)
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        seg = segment_log is not None
        L = _seg_log(segment_log, min(block_size_id, 6)) if seg else 0
        self._flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, (seg and seg_first is None) or max_total_blocks is None or (dst is None and dst_capacity is None))
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, src.device, n * E)
        else:
            sf, nf = None, n * E
        mixed = codecs is not None or isinstance(codec, AutoCodec)
        choose = mixed and codecs is None
        codecs, cgu = _codecs(self, codecs, nf, src.device) if mixed else (None, None)
        max_total_blocks, dst, dst_capacity, g = _frames_room(self, shost, n, E, nf, block_size_id, max_total_blocks, dst, dst_capacity, align_log, src.device)
        planes = _split_room(self, planes, src, capacity, True)
        foff = _i64(self, frame_offsets, nf + 1, src.device, "frame_offsets")
        fres = _i64(self, frame_results, nf, src.device, "frame_results")
        tres = _i64(self, tensor_results, n, src.device, "tensor_results")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        so = _i64(self, seg_offsets, nf + 1, src.device, "seg_offsets") if seg else None
        workspace = _writer_workspace(self, workspace, nf, max_total_blocks, block_size_id, codec, mixed, choose, src.device)
        tol = codec.tolerance_permille if choose and isinstance(codec, AutoCodec) else 0
        head = (_ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src), _ptr(soff), SZ(n), C.c_uint(E), C.c_uint64(capacity))
        writer = (SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(0 if mixed else codec),
                  _ptr((codecs if codecs.numel() else codecs.new_zeros(1)) if mixed else None), C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(tol),
                  C.c_uint(align_log), _ptr(planes), _ptr(poff))
        tail = (_ptr(workspace), SZ(workspace.numel()), *st, _stream())
        if seg:
            call = self.lib.FSEHIP_tensor_compress_seg_pred_dbatch if stride is _NO_STRIDE else self.lib.FSEHIP_tensor_compress_seg_pred_stride_dbatch
            _check(call(*head, _ptr(sf), SZ(nf), C.c_uint(L), *writer, _ptr(so), *tail), what)
        else:
            call = self.lib.FSEHIP_tensor_compress_pred_dbatch if stride is _NO_STRIDE else self.lib.FSEHIP_tensor_compress_pred_stride_dbatch
            _check(call(*head, *writer, *tail), what)
        _check_codecs(cgu, nf, what)
        if g is not None:
            g.check(what)
        return dst, foff, fres, tres, (codecs[:nf] if mixed else None)

    def tensor_compress_pred_dbatch(self, src, src_offsets, elem_bytes, codec=0, codecs=None, block_size_id=5, capacity=None, dst=None, dst_capacity=None,
                                    max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None, plane_offsets=None,
                                    workspace=None):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs): planes_split_pred_dbatch, then the packed writer over the planes --
        frame i*E+p is the .fse frame of plane p of the neighbour differences of tensor i.  codec / codecs as tensor_compress_seg_dbatch takes
        them (0 / 1, an AutoCodec, or a codec per frame given).  planes (for every elem_bytes) and plane_offsets (n*E+1) are scratch; the
        workspace is the (mixed) writer's for n*E frames.  With everything given the call is launches only."""
        return _compress_pred(self, "tensor_compress_pred_dbatch", src, src_offsets, elem_bytes, None, None, None, codec, codecs, block_size_id, capacity, dst,
                              dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, None, workspace)

    def tensor_compress_seg_pred_dbatch(self, src, src_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None, codec=0, codecs=None, block_size_id=5,
                                        capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None,
                                        tensor_results=None, planes=None, plane_offsets=None, seg_offsets=None, workspace=None):
        """tensor_compress_seg_dbatch of the neighbour differences: a run of 1024 elements divides every segment, so the frames are one per
        segment of the predicted planes with no rule of their own."""
        return _compress_pred(self, "tensor_compress_seg_pred_dbatch", src, src_offsets, elem_bytes, segment_log, seg_first, n_segments, codec, codecs, block_size_id,
                              capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, seg_offsets,
                              workspace)

    def _decompress_pred(self, what, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first, n_segments, dst, dst_capacity, max_total_blocks, planes,
                         planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace, results, stride=_NO_STRIDE):
        st = () if stride is _NO_STRIDE else _stride(stride, what)               # (the _pred_ exports take none)
        E = _elem(elem_bytes)
        seg = segment_log is not None
        L = _seg_log(segment_log) if seg else 0
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None or planes is None or (seg and seg_first is None))
        n = doff.numel() - 1
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(dhost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, frames.device, n * E)
        else:
            sf, nf = None, n * E
        if foff.numel() != nf + 1:
            raise ValueError("frame_offsets: one entry per frame (%d) and one more" % nf)
        if max_total_blocks is None:
            _, bfirst = self.frame_plan_dbatch(frames, foff, None, 0)
            max_total_blocks = int(bfirst[nf].item())
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, None if planes is not None else int(dhost[-1]), frames.device)
        poff = _i64(self, plane_offsets, n * E + 1, frames.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, frames.device, "plane_sizes")
        res = _i64(self, results, n, frames.device, "results")
        workspace = _reader_workspace(self, workspace, nf, max_total_blocks, frames.device)
        head = (_ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(res), _ptr(frames), _ptr(foff), SZ(n), C.c_uint(E))
        tail = (_ptr(poff), _ptr(psz), _ptr(workspace), SZ(workspace.numel()), *st, _stream())
        if seg:
            so = _i64(self, seg_offsets, nf + 1, frames.device, "seg_offsets")
            sres = _i64(self, seg_results, nf, frames.device, "seg_results")
            call = self.lib.FSEHIP_tensor_decompress_seg_pred_dbatch if stride is _NO_STRIDE else self.lib.FSEHIP_tensor_decompress_seg_pred_stride_dbatch
            _check(call(*head, _ptr(sf), SZ(nf), C.c_uint(L), SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(so), _ptr(sres), *tail), what)
        else:
            call = self.lib.FSEHIP_tensor_decompress_pred_dbatch if stride is _NO_STRIDE else self.lib.FSEHIP_tensor_decompress_pred_stride_dbatch
            _check(call(*head, SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), *tail), what)
        if g is not None:
            g.check(what)
        return dst, res

    def tensor_decompress_pred_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, dst=None, dst_capacity=None, max_total_blocks=None, planes=None,
                                      planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None, results=None):
        """tensor_decompress_dbatch of frames that tensor_compress_pred_dbatch wrote: the packed reader into `planes`, then
        planes_merge_pred_dbatch.  The frames do not say that they hold differences."""
        return _decompress_pred(self, "tensor_decompress_pred_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, None, None, None, dst, dst_capacity,
                                max_total_blocks, planes, planes_capacity, None, None, plane_offsets, plane_results, workspace, results)

    def tensor_decompress_seg_pred_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first=None, n_segments=None, dst=None,
                                          dst_capacity=None, max_total_blocks=None, planes=None, planes_capacity=None, seg_offsets=None, seg_results=None,
                                          plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_seg_dbatch of frames that tensor_compress_seg_pred_dbatch wrote: the packed reader, the fold, then
        planes_merge_pred_dbatch."""
        return _decompress_pred(self, "tensor_decompress_seg_pred_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first, n_segments, dst,
                                dst_capacity, max_total_blocks, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace, results)

    for f in (planes_split_pred_dbatch, planes_merge_pred_dbatch, tensor_compress_pred_dbatch, tensor_decompress_pred_dbatch, tensor_compress_seg_pred_dbatch,
              tensor_decompress_seg_pred_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- strided predicted planes (csrc/planes_stride.hip; fsehip.h "strided predicted planes"): the predecessor `stride` elements back, the
    # same channel of interleaved data.  The six calls above with `stride` (1 .. 8, required) behind elem_bytes; stride 1 is those calls
    def planes_split_pred_stride_dbatch(self, src, src_offsets, elem_bytes, stride, capacity=None, planes=None, plane_offsets=None, results=None):
        """planes_split_pred_dbatch with the predecessor `stride` elements in front, 0 for the first `stride` elements of every run."""
        return planes_split_pred_dbatch(self, src, src_offsets, elem_bytes, capacity, planes, plane_offsets, results, _stride_arg=stride)

    def planes_merge_pred_stride_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, stride, dst=None, capacity=None, results=None):
        """planes_merge_pred_dbatch, the `stride` interleaved chains of every run summed back: the inverse of planes_split_pred_stride_dbatch."""
        return planes_merge_pred_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, dst, capacity, results, _stride_arg=stride)

    def tensor_compress_pred_stride_dbatch(self, src, src_offsets, elem_bytes, stride, codec=0, codecs=None, block_size_id=5, capacity=None, dst=None,
                                           dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None,
                                           planes=None, plane_offsets=None, workspace=None):
        """tensor_compress_pred_dbatch over planes_split_pred_stride_dbatch.  The frames do not record the stride; the caller carries it."""
        return _compress_pred(self, "tensor_compress_pred_stride_dbatch", src, src_offsets, elem_bytes, None, None, None, codec, codecs, block_size_id, capacity, dst,
                              dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets, None, workspace, stride)

    def tensor_compress_seg_pred_stride_dbatch(self, src, src_offsets, elem_bytes, stride, segment_log, seg_first=None, n_segments=None, codec=0, codecs=None,
                                               block_size_id=5, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None,
                                               frame_results=None, tensor_results=None, planes=None, plane_offsets=None, seg_offsets=None, workspace=None):
        """tensor_compress_seg_pred_dbatch over planes_split_pred_stride_dbatch: runs stay 1024 elements whatever the stride, a segment starts on one."""
        return _compress_pred(self, "tensor_compress_seg_pred_stride_dbatch", src, src_offsets, elem_bytes, segment_log, seg_first, n_segments, codec, codecs,
                              block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes, plane_offsets,
                              seg_offsets, workspace, stride)

    def tensor_decompress_pred_stride_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, stride, dst=None, dst_capacity=None, max_total_blocks=None,
                                             planes=None, planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None, results=None):
        """tensor_decompress_pred_dbatch of frames that tensor_compress_pred_stride_dbatch wrote with the same stride."""
        return _decompress_pred(self, "tensor_decompress_pred_stride_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, None, None, None, dst, dst_capacity,
                                max_total_blocks, planes, planes_capacity, None, None, plane_offsets, plane_results, workspace, results, stride)

    def tensor_decompress_seg_pred_stride_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, stride, segment_log, seg_first=None, n_segments=None, dst=None,
                                                 dst_capacity=None, max_total_blocks=None, planes=None, planes_capacity=None, seg_offsets=None, seg_results=None,
                                                 plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_seg_pred_dbatch of frames that tensor_compress_seg_pred_stride_dbatch wrote with the same stride."""
        return _decompress_pred(self, "tensor_decompress_seg_pred_stride_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, segment_log, seg_first, n_segments,
                                dst, dst_capacity, max_total_blocks, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace, results,
                                stride)

    for f in (planes_split_pred_stride_dbatch, planes_merge_pred_stride_dbatch, tensor_compress_pred_stride_dbatch, tensor_decompress_pred_stride_dbatch,
              tensor_compress_seg_pred_stride_dbatch, tensor_decompress_seg_pred_stride_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- tensor digests and checked deltas (csrc/planes_digest.hip; fsehip.h "tensor digests and checked deltas"): a 64-bit digest per
    # tensor at the memory rate, and the gate that turns a digest mismatch into frames every reader refuses
    def tensor_digest_workspace_bound(self, capacity, n_tensors):
        """the workspace of tensor_digest_dbatch for n_tensors tensors inside `capacity` bytes.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_tensor_digest_workspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_tensor_digest_workspaceBound(C.c_uint64(int(capacity)), SZ(int(n_tensors))))
        if r >= (1 << 62):
            raise ValueError("tensor_digest_workspace_bound(%r, %r)" % (capacity, n_tensors))
        return r

    def tensor_digest_dbatch(self, src, src_offsets, capacity=None, digests=None, results=None, workspace=None):
        """-> (digests, results): digests[i] = the 64-bit digest of tensor i = src[src_offsets[i] : src_offsets[i+1]] as an int64 (the same 64
        bits; & (2**64 - 1) gives the unsigned value), results[i] = its size; a slot whose offsets decrease or that ends behind `capacity`
        (default: src's size) gets -1 and digest 0.  The digest depends on the tensor's bytes alone, not on where it lies.  With src_offsets
        on the device and digests, results and workspace given the call is launches only."""
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        dig = _i64(self, digests, n, src.device, "digests")
        res = _i64(self, results, n, src.device, "results")
        if workspace is None:
            workspace = torch.empty(max(tensor_digest_workspace_bound(self, capacity, n), 1), dtype=torch.uint8, device=src.device)
        _check(self.lib.FSEHIP_tensor_digest_dbatch(_ptr(dig), _ptr(res), VP(src.data_ptr() or workspace.data_ptr()), _ptr(soff), SZ(n), C.c_uint64(capacity),
                                                    _ptr(workspace), SZ(workspace.numel()), _stream()), "tensor_digest_dbatch")
        return dig, res

    def tensor_gate_dbatch(self, frame_offsets, digests, digest_results, expected, elem_bytes, frame_first=None, n_frames=None, gated_offsets=None, results=None):
        """-> (gated_offsets, results): frame_offsets with every frame of a tensor whose digest is not the expected one (or whose digest result
        is an error) turned into an empty extent at the start of the next tensor's first frame -- the readers answer those with -3
        (srcSize_wrong) and the tensor keeps its bytes; the frames of the others are unchanged.  results[i] = digest_results[i] for a tensor that
        passes, the digest's error, or -4 (corruption_detected) for a mismatch.  Tensor i owns the frames i*E .. (i+1)*E - 1, or with
        frame_first (the seg_first of a segmented object) frame_first[i*E] .. frame_first[(i+1)*E] - 1.  gated_offsets goes wherever
        frame_offsets goes in the reading calls.  digests / expected: int64 tensors of the 64 bits (tensor_digest_dbatch), or sequences of ints."""
        E = _elem(elem_bytes)
        foff, _ = self._offsets(frame_offsets, torch.device("cuda") if not isinstance(frame_offsets, torch.Tensor) else frame_offsets.device, False)
        device = foff.device
        nf = foff.numel() - 1 if n_frames is None else int(n_frames)
        if nf < 0 or nf + 1 > foff.numel():
            raise ValueError("frame_offsets: %d entries for %d frames" % (foff.numel(), nf))

        def bits(t, what):
            if isinstance(t, torch.Tensor):
                return _i64(self, t, 0, device, what)
            a = np.asarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in t], dtype=np.uint64).astype(np.int64)
            return torch.from_numpy(a).to(device)
        dig, exp = bits(digests, "digests"), bits(expected, "expected")
        n = exp.numel()
        dres = _i64(self, digest_results, n, device, "digest_results")
        if dig.numel() < n:
            raise ValueError("digests: %d entries for %d tensors" % (dig.numel(), n))
        sf = None
        if frame_first is not None:
            sf, _ = _seg_first(self, frame_first, nf, device, n * E)
        elif nf != n * E:
            raise ValueError("frame_offsets: %d frames for %d tensors of %d planes" % (nf, n, E))
        gated = _i64(self, gated_offsets, nf + 1, device, "gated_offsets")
        res = _i64(self, results, n, device, "results")
        some = gated if n == 0 else None                      # (arrays of no entries still need an address)
        _check(self.lib.FSEHIP_tensor_gate_dbatch(_ptr(gated), _ptr(some if some is not None else res), _ptr(foff), SZ(nf), _ptr(sf), C.c_uint(E),
                                                  _ptr(some if some is not None else dig), _ptr(some if some is not None else dres),
                                                  _ptr(some if some is not None else exp), SZ(n), _stream()), "tensor_gate_dbatch")
        return gated, res

    def tensor_digests(self, tensors):
        """-> one int (0 .. 2**64 - 1) per tensor: the digest of its contiguous bytes (tensor_digest_dbatch; fsehip.h "tensor digests and checked
        deltas").  CUDA tensors of any dtype, shape and device; the tensors of a device are digested in one call over their concatenated
        bytes, and the values do not depend on that grouping.  Not cryptographic.  A single tensor of a device is digested where it
        lies; the concatenation of several is a copy -- one more read and write
        of the bytes around a kernel that runs at the memory rate: a caller whose tensors already lie in one flat resident buffer calls
        tensor_digest_dbatch on it with their offsets, which copies nothing."""
        tensors = list(tensors)
        for t in tensors:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError("tensor_digests takes CUDA tensors")
        out = [None] * len(tensors)
        for device in sorted({t.device for t in tensors}, key=str):
            idx = [i for i, t in enumerate(tensors) if t.device == device]
            with torch.cuda.device(device):
                for i, d in zip(idx, _group_digests(self, [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx], device)):
                    out[i] = d
        return out

    def _group_digests(self, raw, device, src=None):
        """the digests of the flat uint8 tensors `raw` (src: their concatenation, where the caller has it) as ints"""
        offs = np.concatenate([[0], np.cumsum([r.numel() for r in raw])]).astype(np.uint64)
        if src is None:
            src = raw[0] if len(raw) == 1 and raw[0].numel() else torch.cat(raw) if int(offs[-1]) else torch.zeros(1, dtype=torch.uint8, device=device)[:0]
        dig, res = tensor_digest_dbatch(self, src, offs)
        got = torch.cat([dig, res]).cpu().tolist()
        n = len(raw)
        if got[n:] != [int(x) for x in np.diff(offs.astype(np.int64))]:
            raise RuntimeError("tensor_digests: results %s" % (got[n:n + 8],))
        return [d & 0xFFFFFFFFFFFFFFFF for d in got[:n]]

    for f in (tensor_digest_workspace_bound, tensor_digest_dbatch, tensor_gate_dbatch, tensor_digests):
        setattr(FseHip, f.__name__, f)

    # ---- plane estimates (csrc/planes_estimate.hip; fsehip.h "plane estimates"): per tensor and candidate transform the order-0 cost of
    # every plane from one read of the tensors, an estimated size and a choice
    def planes_estimate_workspace_bound(self, n_tensors, elem_bytes, candidate_mask):
        """the workspace of planes_estimate_dbatch: per tensor and requested candidate elem_bytes histograms of 256 counters.  Host
        arithmetic: needs no device."""
        self.lib.FSEHIP_planes_estimate_workspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_planes_estimate_workspaceBound(SZ(int(n_tensors)), C.c_uint(int(elem_bytes)), C.c_uint(int(candidate_mask) & 0xFFFFFFFF)))
        if r >= (1 << 62):
            raise ValueError("planes_estimate_workspace_bound(%r, %r, %r)" % (n_tensors, elem_bytes, candidate_mask))
        return r

    def planes_estimate_dbatch(self, src, src_offsets, elem_bytes, candidate_mask=3, margin_permille=50, base=None, capacity=None, plane_bits=None, est_bytes=None,
                               choice=None, results=None, workspace=None):
        """-> (plane_bits, est_bytes, choice, results) for tensor i = src[src_offsets[i] : src_offsets[i+1]] and candidate c (bit 1 << c of
        candidate_mask; 0 plain, 1 pred, 2 xor, 3 sub -- the last two need `base`, laid out as src is): plane_bits[(i*4+c)*E+p] = the
        order-0 cost of plane p in 1/256 bits, est_bytes[i*4+c] = the estimated bytes of the tensor, choice[i] (uint8) = the chosen
        candidate under margin_permille, results[i] = its size.  int64 tensors of the library's 64 bits: a slot of a candidate that was
        not requested, or of a refused tensor (results -1: its offsets decrease or it ends behind `capacity`, default src's size; -3: it
        holds 2^32 bytes or more; choice 0xFF), reads -1.  src and base are only read.  With src_offsets on the device and the outputs
        and the workspace given the call is launches only and can be captured into a graph; it zeroes its workspace itself."""
        E = _elem(elem_bytes)
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        need = planes_estimate_workspace_bound(self, n, E, candidate_mask)
        pb = _i64(self, plane_bits, n * 4 * E, src.device, "plane_bits")
        eb = _i64(self, est_bytes, n * 4, src.device, "est_bytes")
        ch = torch.zeros(max(n, 1), dtype=torch.uint8, device=src.device)[:n] if choice is None else _u8(choice, n, src.device, "choice")
        res = _i64(self, results, n, src.device, "results")
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
        _check(self.lib.FSEHIP_planes_estimate_dbatch(_ptr(pb), _ptr(eb), _ptr(ch), _ptr(res), VP(src.data_ptr() or workspace.data_ptr()), _ptr(base), _ptr(soff), SZ(n),
                                                      C.c_uint(E), C.c_uint64(capacity), C.c_uint(int(candidate_mask)), C.c_uint(int(margin_permille)), _ptr(workspace),
                                                      SZ(workspace.numel()), _stream()), "planes_estimate_dbatch")
        return pb, eb, ch, res

    for f in (planes_estimate_workspace_bound, planes_estimate_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- a transform per tensor (csrc/planes_each.hip, capi_each.hip; fsehip.h "a transform per tensor"): the split, the merge and the
    # composites with the transform of tensor i read from a device array -- given, or chosen by the estimate inside the call and returned
    def _transforms(transforms, n, device):
        """the `transforms` of a call that takes them as given: a CUDA uint8 tensor of n ids (handed on as it is: the device refuses a
        byte that is none of the four), or a sequence of n names / ids -> the CUDA uint8 tensor"""
        if isinstance(transforms, torch.Tensor):
            return _u8(transforms, n, device, "transforms")
        ids = [EST_NAMES.index(t) if isinstance(t, str) and t in EST_NAMES else t for t in transforms]
        if len(ids) != n or any(not isinstance(t, numbers.Integral) or isinstance(t, bool) or not 0 <= t <= 255 for t in ids):
            raise ValueError("transforms: %d names out of %r (or ids 0 .. 255) are needed" % (n, EST_NAMES))
        return torch.tensor(ids, dtype=torch.uint8).to(device) if n else torch.zeros(1, dtype=torch.uint8, device=device)[:0]

    def _strides(strides, n, device):
        """the `strides` of a call that takes them as given: None (stride 1 everywhere), a CUDA uint8 tensor of n bytes (handed on as it
        is: the device refuses a pred tensor whose byte is 0 or above 8), or a sequence of n integers 0 .. 255 -> the CUDA uint8 tensor"""
        if strides is None:
            return None
        if isinstance(strides, torch.Tensor):
            return _u8(strides, n, device, "strides")
        ids = list(strides)
        if len(ids) != n or any(not isinstance(t, numbers.Integral) or isinstance(t, bool) or not 0 <= t <= 255 for t in ids):
            raise ValueError("strides: %d integers (1 .. %d for a pred tensor) are needed" % (n, PRED_MAX_STRIDE))
        return torch.tensor([int(t) for t in ids], dtype=torch.uint8).to(device) if n else torch.zeros(1, dtype=torch.uint8, device=device)[:0]

    def _stride_mask(strides, what):
        """a candidate set of strides, integers out of 1 .. 8 (or the mask itself, an integer 1 .. 255) -> the strideMask of the C calls"""
        if isinstance(strides, numbers.Integral) and not isinstance(strides, bool):
            if not 1 <= strides <= 255:
                raise ValueError("%s: stride mask %r, bits 0 .. 7 and at least one are needed" % (what, strides))
            return int(strides)
        mask = 0
        for st in ([] if isinstance(strides, str) else list(strides)):
            _stride(st, what)
            mask |= 1 << (int(st) - 1)
        if not mask:
            raise ValueError("%s: strides %r, integers out of 1 .. %d are needed" % (what, strides, PRED_MAX_STRIDE))
        return mask

    def tensor_each_stride_workspace_head(self, n_tensors, elem_bytes, choose, candidate_mask=3, stride_mask=1):
        """tensor_each_workspace_head of the _each_stride_ composites: with stride_mask 1 the same number."""
        self.lib.FSEHIP_tensor_each_stride_workspaceHead.restype = SZ
        r = int(self.lib.FSEHIP_tensor_each_stride_workspaceHead(SZ(int(n_tensors)), C.c_uint(int(elem_bytes)), C.c_int(1 if choose else 0),
                                                                 C.c_uint(int(candidate_mask) & 0xFFFFFFFF), C.c_uint(int(stride_mask) & 0xFFFFFFFF)))
        if r >= (1 << 62):
            raise ValueError("tensor_each_stride_workspace_head(%r, %r, %r, %r, %r)" % (n_tensors, elem_bytes, choose, candidate_mask, stride_mask))
        return r

    def tensor_each_workspace_head(self, n_tensors, elem_bytes, choose, candidate_mask=3):
        """the bytes of a tensor_compress_each_dbatch workspace that lie in front of the writer's own: 0 with the transforms given, the
        estimate's counters and outputs where the call chooses.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_tensor_each_workspaceHead.restype = SZ
        r = int(self.lib.FSEHIP_tensor_each_workspaceHead(SZ(int(n_tensors)), C.c_uint(int(elem_bytes)), C.c_int(1 if choose else 0),
                                                          C.c_uint(int(candidate_mask) & 0xFFFFFFFF)))
        if r >= (1 << 62):
            raise ValueError("tensor_each_workspace_head(%r, %r, %r, %r)" % (n_tensors, elem_bytes, choose, candidate_mask))
        return r

    def planes_split_each_dbatch(self, src, src_offsets, elem_bytes, transforms, base=None, capacity=None, planes=None, plane_offsets=None, results=None,
                                 _strides_arg=_NO_STRIDE):
        """-> (planes, plane_offsets, results): tensor i split as transforms[i] says (0 plain, 1 pred, 2 xor, 3 sub; names or a CUDA uint8
        tensor) -- byte for byte what planes_split_dbatch, planes_split_pred_dbatch or planes_split_xor_dbatch (delta_op 0 / 1) writes for
        it.  base: laid out as src, read for xor and sub tensors only; a tensor whose byte is none of the four, or xor / sub without a
        base, is refused: results -1, nothing of it read or written.  `planes` is written for every elem_bytes."""
        E = _elem(elem_bytes)
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        tr = _transforms(transforms, n, src.device)
        what = "planes_split_each_dbatch" if _strides_arg is _NO_STRIDE else "planes_split_each_stride_dbatch"
        held = None if _strides_arg is _NO_STRIDE else _strides(_strides_arg, n, src.device)
        st = () if _strides_arg is _NO_STRIDE else (_ptr(held),)                               # (the _each_ export takes none)
        g = None
        if planes is None:
            planes, g = self._dst(1, src.numel(), src.device)
            planes = planes[0]
        elif _room(self, planes, None, "planes") < capacity:
            raise ValueError("planes holds %d bytes, the capacity is %d" % (planes.numel(), capacity))
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        res = _i64(self, results, n, src.device, "results")
        call = self.lib.FSEHIP_planes_split_each_dbatch if _strides_arg is _NO_STRIDE else self.lib.FSEHIP_planes_split_each_stride_dbatch
        _check(call(_ptr(planes), _ptr(poff), _ptr(res), _ptr(src), _ptr(base), VP(tr.data_ptr() or res.data_ptr()), *st, _ptr(soff), SZ(n), C.c_uint(E),
                    C.c_uint64(capacity), _stream()), what)
        if g is not None:
            g.check(what)
        return planes, poff, res

    def planes_merge_each_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, transforms, base=None, dst=None, capacity=None, results=None,
                                 _strides_arg=_NO_STRIDE):
        """-> (dst, results): the inverse of planes_split_each_dbatch with the merges' results and rules.  base may be dst itself (the
        resident tensors are updated where they lie; a plain or pred tensor overwrites its bytes, a refused one keeps them).  dst must not
        overlap planes."""
        E = _elem(elem_bytes)
        self._flat(planes, "planes")
        doff, dhost = self._offsets(dst_offsets, planes.device, dst is None)
        n = doff.numel() - 1
        poff = _i64(self, plane_offsets, n * E, planes.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, planes.device, "plane_sizes")
        dst, capacity, g = _dst_room(self, dst, capacity, dhost, planes.device)
        _base(self, base, planes, capacity, "dst")
        tr = _transforms(transforms, n, planes.device)
        res = _i64(self, results, n, planes.device, "results")
        what = "planes_merge_each_dbatch" if _strides_arg is _NO_STRIDE else "planes_merge_each_stride_dbatch"
        held = None if _strides_arg is _NO_STRIDE else _strides(_strides_arg, n, planes.device)
        st = () if _strides_arg is _NO_STRIDE else (_ptr(held),)                               # (the _each_ export takes none)
        call = self.lib.FSEHIP_planes_merge_each_dbatch if _strides_arg is _NO_STRIDE else self.lib.FSEHIP_planes_merge_each_stride_dbatch
        _check(call(_ptr(dst), _ptr(doff), _ptr(res), _ptr(planes), _ptr(poff), _ptr(psz), _ptr(base), VP(tr.data_ptr() or res.data_ptr()), *st, SZ(n), C.c_uint(E),
                    C.c_uint64(capacity), _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    def _compress_each(self, what, src, src_offsets, elem_bytes, transforms, base, candidate_mask, margin_permille, est_bytes, segment_log, seg_first, n_segments, codec,
                       codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results, planes,
                       plane_offsets, seg_offsets, workspace, chosen, strides=_NO_STRIDE, stride_mask=None, chosen_strides=None):
        """strides is _NO_STRIDE: the _each_ exports.  Else the _each_stride_ exports: `strides` as _strides takes them where the transforms are
        given; where the call chooses, stride_mask is the candidate set and the chosen strides are returned (in chosen_strides where given)"""
        each = strides is _NO_STRIDE
        E = _elem(elem_bytes)
        align_log = _align_log(align_log)
        seg = segment_log is not None
        L = _seg_log(segment_log, min(block_size_id, 6)) if seg else 0
        self._flat(src, "src")
        soff, shost = self._offsets(src_offsets, src.device, (seg and seg_first is None) or max_total_blocks is None or (dst is None and dst_capacity is None))
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        pick = transforms is None                               # the call chooses and returns the choice
        if pick and candidate_mask is None:
            candidate_mask = 3 if base is None else 15
        if not pick:
            tr = _transforms(transforms, n, src.device)
        else:
            tr = torch.zeros(max(n, 1), dtype=torch.uint8, device=src.device)[:n] if chosen is None else _u8(chosen, n, src.device, "chosen")[:n]
        eb = None if est_bytes is None else _i64(self, est_bytes, n * 4, src.device, "est_bytes")
        st, smask = None, 1
        if not each and pick:
            smask = _stride_mask(1 if stride_mask is None else stride_mask, what)
            if smask != 1 and not (candidate_mask >> 1) & 1:
                raise ValueError(what + ": strides are candidates of \"pred\", which is not among the candidates")
            st = torch.ones(max(n, 1), dtype=torch.uint8, device=src.device)[:n] if chosen_strides is None else _u8(chosen_strides, n, src.device, "chosen_strides")[:n]
        elif not each:
            st = _strides(strides, n, src.device)
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(shost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, src.device, n * E)
        else:
            sf, nf = None, n * E
        mixed = codecs is not None or isinstance(codec, AutoCodec)
        choose = mixed and codecs is None
        codecs, cgu = _codecs(self, codecs, nf, src.device) if mixed else (None, None)
        max_total_blocks, dst, dst_capacity, g = _frames_room(self, shost, n, E, nf, block_size_id, max_total_blocks, dst, dst_capacity, align_log, src.device)
        planes = _split_room(self, planes, src, capacity, True)
        foff = _i64(self, frame_offsets, nf + 1, src.device, "frame_offsets")
        fres = _i64(self, frame_results, nf, src.device, "frame_results")
        tres = _i64(self, tensor_results, n, src.device, "tensor_results")
        poff = _i64(self, plane_offsets, n * E + 1, src.device, "plane_offsets")
        so = _i64(self, seg_offsets, nf + 1, src.device, "seg_offsets") if seg else None
        if workspace is None:
            need = (tensor_each_workspace_head(self, n, E, pick, candidate_mask or 0) if each else
                    tensor_each_stride_workspace_head(self, n, E, pick, candidate_mask or 0, smask)) + _writer_need(self, nf, max_total_blocks, block_size_id, codec, mixed, choose)
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
        tol = codec.tolerance_permille if choose and isinstance(codec, AutoCodec) else 0
        sp = () if each else (VP((st.data_ptr() or tres.data_ptr()) if st is not None else None),)
        sm = () if each else (C.c_uint(smask),)
        head = (_ptr(dst), C.c_uint64(int(dst_capacity)), _ptr(foff), _ptr(fres), _ptr(tres), _ptr(src), _ptr(base), VP(tr.data_ptr() or tres.data_ptr()), *sp,
                C.c_int(1 if pick else 0), C.c_uint(int(candidate_mask or 0)), *sm, C.c_uint(int(margin_permille)), _ptr(eb), _ptr(soff), SZ(n), C.c_uint(E),
                C.c_uint64(capacity))
        writer = (SZ(max_total_blocks), C.c_uint(block_size_id), C.c_int(0 if mixed else codec),
                  _ptr((codecs if codecs.numel() else codecs.new_zeros(1)) if mixed else None), C.c_int(CODECS_CHOOSE if choose else CODECS_GIVEN), C.c_uint(tol),
                  C.c_uint(align_log), _ptr(planes), _ptr(poff))
        tail = (_ptr(workspace), SZ(workspace.numel()), _stream())
        if seg:
            call = self.lib.FSEHIP_tensor_compress_seg_each_dbatch if each else self.lib.FSEHIP_tensor_compress_seg_each_stride_dbatch
            _check(call(*head, _ptr(sf), SZ(nf), C.c_uint(L), *writer, _ptr(so), *tail), what)
        else:
            call = self.lib.FSEHIP_tensor_compress_each_dbatch if each else self.lib.FSEHIP_tensor_compress_each_stride_dbatch
            _check(call(*head, *writer, *tail), what)
        _check_codecs(cgu, nf, what)
        if g is not None:
            g.check(what)
        out = (dst, foff, fres, tres, (codecs[:nf] if mixed else None), tr)
        return out if each else out + (st,)

    def tensor_compress_each_dbatch(self, src, src_offsets, elem_bytes, transforms=None, base=None, candidate_mask=None, margin_permille=50, est_bytes=None, codec=0,
                                    codecs=None, block_size_id=5, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None,
                                    frame_results=None, tensor_results=None, planes=None, plane_offsets=None, workspace=None, chosen=None):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs, transforms): planes_split_each_dbatch, then the packed (mixed) writer
        -- frame i*E+p is the frame that the dedicated composite writes for plane p of tensor i under transforms[i].  transforms given (names,
        ids or a CUDA uint8 tensor): read.  transforms None: CHOSEN on the device by planes_estimate_dbatch with candidate_mask (default
        plain | pred without a base, all four with one) and margin_permille, with no host read in between, and returned (in `chosen`, a CUDA
        uint8 tensor of n entries, where one is given) -- give them back to a later call.  est_bytes (n*4 int64, optional): the estimates of a choosing call.  codec / codecs as tensor_compress_pred_dbatch
        takes them.  The workspace: tensor_each_workspace_head bytes in front of the (mixed) writer's.  With everything given the call is
        launches only and can be captured into a graph."""
        return _compress_each(self, "tensor_compress_each_dbatch", src, src_offsets, elem_bytes, transforms, base, candidate_mask, margin_permille, est_bytes, None, None,
                              None, codec, codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results, tensor_results,
                              planes, plane_offsets, None, workspace, chosen)

    def tensor_compress_seg_each_dbatch(self, src, src_offsets, elem_bytes, segment_log, transforms=None, base=None, candidate_mask=None, margin_permille=50,
                                        est_bytes=None, seg_first=None, n_segments=None, codec=0, codecs=None, block_size_id=5, capacity=None, dst=None,
                                        dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None,
                                        planes=None, plane_offsets=None, seg_offsets=None, workspace=None, chosen=None):
        """tensor_compress_each_dbatch with a frame per segment of every plane, as tensor_compress_seg_pred_dbatch cuts them."""
        return _compress_each(self, "tensor_compress_seg_each_dbatch", src, src_offsets, elem_bytes, transforms, base, candidate_mask, margin_permille, est_bytes,
                              segment_log, seg_first, n_segments, codec, codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                              frame_results, tensor_results, planes, plane_offsets, seg_offsets, workspace, chosen)

    def _decompress_each(self, what, frames, frame_offsets, dst_offsets, elem_bytes, transforms, base, segment_log, seg_first, n_segments, dst, dst_capacity,
                         max_total_blocks, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace, results, strides=_NO_STRIDE):
        each = strides is _NO_STRIDE                            # the _each_ exports take no strides
        E = _elem(elem_bytes)
        seg = segment_log is not None
        L = _seg_log(segment_log) if seg else 0
        self._flat(frames, "frames")
        foff, _ = self._offsets(frame_offsets, frames.device, False)
        doff, dhost = self._offsets(dst_offsets, frames.device, dst is None or planes is None or (seg and seg_first is None))
        n = doff.numel() - 1
        if seg:
            if seg_first is None:
                seg_first = planes_segment_first(self, np.diff(dhost.astype(np.int64)).clip(min=0), E, L)
            sf, nf = _seg_first(self, seg_first, n_segments, frames.device, n * E)
        else:
            sf, nf = None, n * E
        if foff.numel() != nf + 1:
            raise ValueError("frame_offsets: one entry per frame (%d) and one more" % nf)
        if max_total_blocks is None:
            _, bfirst = self.frame_plan_dbatch(frames, foff, None, 0)
            max_total_blocks = int(bfirst[nf].item())
        dst, dst_capacity, g = _dst_room(self, dst, dst_capacity, dhost, frames.device)
        _base(self, base, frames, dst_capacity, "dst")
        tr = _transforms(transforms, n, frames.device)
        planes, planes_capacity = _planes_room(self, planes, planes_capacity, None if planes is not None else int(dhost[-1]), frames.device)
        poff = _i64(self, plane_offsets, n * E + 1, frames.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, frames.device, "plane_sizes")
        res = _i64(self, results, n, frames.device, "results")
        workspace = _reader_workspace(self, workspace, nf, max_total_blocks, frames.device)
        held = None if each else _strides(strides, n, frames.device)
        sp = () if each else (_ptr(held),)
        head = (_ptr(dst), _ptr(doff), C.c_uint64(dst_capacity), _ptr(base), VP(tr.data_ptr() or res.data_ptr()), *sp, _ptr(res), _ptr(frames), _ptr(foff), SZ(n),
                C.c_uint(E))
        tail = (_ptr(poff), _ptr(psz), _ptr(workspace), SZ(workspace.numel()), _stream())
        if seg:
            so = _i64(self, seg_offsets, nf + 1, frames.device, "seg_offsets")
            sres = _i64(self, seg_results, nf, frames.device, "seg_results")
            call = self.lib.FSEHIP_tensor_decompress_seg_each_dbatch if each else self.lib.FSEHIP_tensor_decompress_seg_each_stride_dbatch
            _check(call(*head, _ptr(sf), SZ(nf), C.c_uint(L), SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), _ptr(so), _ptr(sres), *tail), what)
        else:
            call = self.lib.FSEHIP_tensor_decompress_each_dbatch if each else self.lib.FSEHIP_tensor_decompress_each_stride_dbatch
            _check(call(*head, SZ(max_total_blocks), _ptr(planes), C.c_uint64(planes_capacity), *tail), what)
        if g is not None:
            g.check(what)
        return dst, res

    def tensor_decompress_each_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, transforms, base=None, dst=None, dst_capacity=None, max_total_blocks=None,
                                      planes=None, planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None, results=None):
        """tensor_decompress_dbatch of frames that tensor_compress_each_dbatch wrote with these transforms (always given here): the packed
        reader into `planes`, then planes_merge_each_dbatch.  base (may be dst: in place) for xor and sub tensors."""
        return _decompress_each(self, "tensor_decompress_each_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, transforms, base, None, None, None, dst,
                                dst_capacity, max_total_blocks, planes, planes_capacity, None, None, plane_offsets, plane_results, workspace, results)

    def tensor_decompress_seg_each_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, transforms, base=None, seg_first=None, n_segments=None,
                                          dst=None, dst_capacity=None, max_total_blocks=None, planes=None, planes_capacity=None, seg_offsets=None, seg_results=None,
                                          plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_seg_dbatch of frames that tensor_compress_seg_each_dbatch wrote: the packed reader, the fold, then
        planes_merge_each_dbatch."""
        return _decompress_each(self, "tensor_decompress_seg_each_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, transforms, base, segment_log, seg_first,
                                n_segments, dst, dst_capacity, max_total_blocks, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace,
                                results)

    # ---- a stride per tensor, strides in the estimate (csrc/planes_each_stride.hip, planes_estimate.hip; fsehip.h, the sections of those names)
    def planes_estimate_stride_workspace_bound(self, n_tensors, elem_bytes, candidate_mask, stride_mask):
        """the workspace of planes_estimate_stride_dbatch; with stride_mask 1 that of planes_estimate_dbatch.  Host arithmetic."""
        self.lib.FSEHIP_planes_estimate_stride_workspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_planes_estimate_stride_workspaceBound(SZ(int(n_tensors)), C.c_uint(int(elem_bytes)), C.c_uint(int(candidate_mask) & 0xFFFFFFFF),
                                                                      C.c_uint(int(stride_mask) & 0xFFFFFFFF)))
        if r >= (1 << 62):
            raise ValueError("planes_estimate_stride_workspace_bound(%r, %r, %r, %r)" % (n_tensors, elem_bytes, candidate_mask, stride_mask))
        return r

    def planes_estimate_stride_dbatch(self, src, src_offsets, elem_bytes, candidate_mask=3, stride_mask=1, margin_permille=50, base=None, capacity=None, plane_bits=None,
                                      est_bytes=None, choice=None, results=None, stride_est_bytes=None, strides=None, workspace=None):
        """-> (plane_bits, est_bytes, choice, results, stride_est_bytes, strides): planes_estimate_dbatch with the pred candidate at every stride
        S whose bit 1 << (S - 1) is set in stride_mask.  stride_est_bytes[i*8+S-1] = the estimate of tensor i at stride S (-1: not
        requested), strides[i] (uint8) = the stride chosen in rising order under margin_permille; the pred slots of plane_bits and
        est_bytes hold the numbers of that stride, and choice is made over those.  A refused tensor: strides 0xFF."""
        E = _elem(elem_bytes)
        self._flat(src, "src")
        soff, _ = self._offsets(src_offsets, src.device, False)
        n = soff.numel() - 1
        capacity = _room(self, src, capacity, "src")
        _base(self, base, src, capacity, "src")
        need = planes_estimate_stride_workspace_bound(self, n, E, candidate_mask, stride_mask)
        pb = _i64(self, plane_bits, n * 4 * E, src.device, "plane_bits")
        eb = _i64(self, est_bytes, n * 4, src.device, "est_bytes")
        ch = torch.zeros(max(n, 1), dtype=torch.uint8, device=src.device)[:n] if choice is None else _u8(choice, n, src.device, "choice")
        res = _i64(self, results, n, src.device, "results")
        seb = _i64(self, stride_est_bytes, n * PRED_MAX_STRIDE, src.device, "stride_est_bytes")
        st = torch.zeros(max(n, 1), dtype=torch.uint8, device=src.device)[:n] if strides is None else _u8(strides, n, src.device, "strides")
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
        _check(self.lib.FSEHIP_planes_estimate_stride_dbatch(_ptr(pb), _ptr(eb), _ptr(ch), _ptr(res), _ptr(seb), VP(st.data_ptr() or workspace.data_ptr()),
                                                             VP(src.data_ptr() or workspace.data_ptr()), _ptr(base), _ptr(soff), SZ(n), C.c_uint(E), C.c_uint64(capacity),
                                                             C.c_uint(int(candidate_mask)), C.c_uint(int(margin_permille)), _ptr(workspace), SZ(workspace.numel()),
                                                             C.c_uint(int(stride_mask)), _stream()), "planes_estimate_stride_dbatch")
        return pb, eb, ch, res, seb, st

    def planes_split_each_stride_dbatch(self, src, src_offsets, elem_bytes, transforms, strides=None, base=None, capacity=None, planes=None, plane_offsets=None,
                                        results=None):
        """planes_split_each_dbatch with strides[i] (1 .. 8) the stride of tensor i where transforms[i] is pred -- the planes of
        planes_split_pred_stride_dbatch at that stride; a 0 or a value above 8 there refuses that tensor alone (results -1).  For every
        other transform the entry is ignored.  strides None: planes_split_each_dbatch."""
        return planes_split_each_dbatch(self, src, src_offsets, elem_bytes, transforms, base, capacity, planes, plane_offsets, results, _strides_arg=strides)

    def planes_merge_each_stride_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, transforms, strides=None, base=None, dst=None, capacity=None,
                                        results=None):
        """the inverse of planes_split_each_stride_dbatch, with the rules of planes_merge_each_dbatch."""
        return planes_merge_each_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, elem_bytes, transforms, base, dst, capacity, results, _strides_arg=strides)

    def tensor_compress_each_stride_dbatch(self, src, src_offsets, elem_bytes, transforms=None, strides=None, base=None, candidate_mask=None, stride_mask=None,
                                           margin_permille=50, est_bytes=None, codec=0, codecs=None, block_size_id=5, capacity=None, dst=None, dst_capacity=None,
                                           max_total_blocks=None, align_log=0, frame_offsets=None, frame_results=None, tensor_results=None, planes=None,
                                           plane_offsets=None, workspace=None, chosen=None, chosen_strides=None):
        """-> (dst, frame_offsets, frame_results, tensor_results, codecs, transforms, strides): tensor_compress_each_dbatch with a stride per
        pred tensor.  transforms given: `strides` is read with them (None: stride 1 everywhere).  transforms None: both are CHOSEN on the
        device by planes_estimate_stride_dbatch with candidate_mask and stride_mask (a mask, or a sequence of strides; default stride 1 alone)
        and returned -- strides 1 for the tensors that did not choose pred."""
        return _compress_each(self, "tensor_compress_each_stride_dbatch", src, src_offsets, elem_bytes, transforms, base, candidate_mask, margin_permille, est_bytes, None,
                              None, None, codec, codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets, frame_results,
                              tensor_results, planes, plane_offsets, None, workspace, chosen, strides, stride_mask, chosen_strides)

    def tensor_compress_seg_each_stride_dbatch(self, src, src_offsets, elem_bytes, segment_log, transforms=None, strides=None, base=None, candidate_mask=None,
                                               stride_mask=None, margin_permille=50, est_bytes=None, seg_first=None, n_segments=None, codec=0, codecs=None,
                                               block_size_id=5, capacity=None, dst=None, dst_capacity=None, max_total_blocks=None, align_log=0, frame_offsets=None,
                                               frame_results=None, tensor_results=None, planes=None, plane_offsets=None, seg_offsets=None, workspace=None, chosen=None,
                                               chosen_strides=None):
        """tensor_compress_each_stride_dbatch with a frame per segment of every plane."""
        return _compress_each(self, "tensor_compress_seg_each_stride_dbatch", src, src_offsets, elem_bytes, transforms, base, candidate_mask, margin_permille, est_bytes,
                              segment_log, seg_first, n_segments, codec, codecs, block_size_id, capacity, dst, dst_capacity, max_total_blocks, align_log, frame_offsets,
                              frame_results, tensor_results, planes, plane_offsets, seg_offsets, workspace, chosen, strides, stride_mask, chosen_strides)

    def tensor_decompress_each_stride_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, transforms, strides=None, base=None, dst=None, dst_capacity=None,
                                             max_total_blocks=None, planes=None, planes_capacity=None, plane_offsets=None, plane_results=None, workspace=None,
                                             results=None):
        """tensor_decompress_each_dbatch of frames that tensor_compress_each_stride_dbatch wrote with these transforms and strides."""
        return _decompress_each(self, "tensor_decompress_each_stride_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, transforms, base, None, None, None, dst,
                                dst_capacity, max_total_blocks, planes, planes_capacity, None, None, plane_offsets, plane_results, workspace, results, strides)

    def tensor_decompress_seg_each_stride_dbatch(self, frames, frame_offsets, dst_offsets, elem_bytes, segment_log, transforms, strides=None, base=None, seg_first=None,
                                                 n_segments=None, dst=None, dst_capacity=None, max_total_blocks=None, planes=None, planes_capacity=None,
                                                 seg_offsets=None, seg_results=None, plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_seg_each_dbatch of frames that tensor_compress_seg_each_stride_dbatch wrote."""
        return _decompress_each(self, "tensor_decompress_seg_each_stride_dbatch", frames, frame_offsets, dst_offsets, elem_bytes, transforms, base, segment_log, seg_first,
                                n_segments, dst, dst_capacity, max_total_blocks, planes, planes_capacity, seg_offsets, seg_results, plane_offsets, plane_sizes, workspace,
                                results, strides)

    for f in (planes_estimate_stride_workspace_bound, planes_estimate_stride_dbatch, tensor_each_stride_workspace_head, planes_split_each_stride_dbatch,
              planes_merge_each_stride_dbatch, tensor_compress_each_stride_dbatch, tensor_compress_seg_each_stride_dbatch, tensor_decompress_each_stride_dbatch,
              tensor_decompress_seg_each_stride_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- windows of tensors with a transform per tensor (fsehip.h, the section of that name): the read side of the windows for frames of
    # tensor_compress_seg_each_dbatch and tensor_compress_seg_pred_dbatch
    def planes_merge_window_each_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, windows, elem_bytes, transforms, base=None, dst=None, capacity=None,
                                        results=None, _strides_arg=_NO_STRIDE):
        """-> (dst, results): planes_merge_each_dbatch of the windows (a, b), in elements, of every tensor: plane_offsets point at the window's
        first byte of every plane and plane_sizes are b - a, as planes_fold_window_dbatch leaves them; slot i of dst_offsets receives
        tensor_i[a * E : b * E].  For a "pred" tensor the a % 1024 plane bytes in front of each of its plane offsets must be the decoded bytes
        in front of the window: they are summed and not stored.  Refused alone, results -1 and nothing written: a byte that is none of the
        four, xor / sub without a base, a > b, a window that disagrees with the plane sizes, a pred tensor whose lead is larger than a
        plane offset.  windows: host pairs or a CUDA int64 tensor of 2 n entries.  base: dst's layout, may be dst."""
        E = _elem(elem_bytes)
        self._flat(planes, "planes")
        doff, dhost = self._offsets(dst_offsets, planes.device, dst is None)
        n = doff.numel() - 1
        poff = _i64(self, plane_offsets, n * E, planes.device, "plane_offsets")
        psz = _i64(self, plane_sizes, n * E, planes.device, "plane_sizes")
        win, _ = _windows(self, windows, planes.device, n)
        dst, capacity, g = _dst_room(self, dst, capacity, dhost, planes.device)
        _base(self, base, planes, capacity, "dst")
        tr = _transforms(transforms, n, planes.device)
        res = _i64(self, results, n, planes.device, "results")
        each = _strides_arg is _NO_STRIDE
        what = "planes_merge_window_each_dbatch" if each else "planes_merge_window_each_stride_dbatch"
        held = None if each else _strides(_strides_arg, n, planes.device)
        st = () if each else (_ptr(held),)                                                       # (the _each_ export takes none)
        call = self.lib.FSEHIP_planes_merge_window_each_dbatch if each else self.lib.FSEHIP_planes_merge_window_each_stride_dbatch
        _check(call(_ptr(_some(dst)), _ptr(doff), _ptr(_some(res)), _ptr(planes), _ptr(_some(poff)), _ptr(_some(psz)), _ptr(base), VP(tr.data_ptr() or doff.data_ptr()), *st,
                    _ptr(_some(win)), SZ(n), C.c_uint(E), C.c_uint64(capacity), _stream()), what)
        if g is not None:
            g.check(what)
        return dst, res

    def tensor_decompress_window_each_dbatch(self, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log, transforms, seg_first=None,
                                             n_segments=None, sel_first=None, n_selected=None, base=None, dst=None, dst_capacity=None, max_total_blocks=None,
                                             block_size_id=5, planes=None, planes_capacity=None, sel_frame_offsets=None, sel_offsets=None, sel_results=None,
                                             plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_window_dbatch for frames that tensor_compress_seg_each_dbatch wrote with these transforms (names, ids or a CUDA
        uint8 tensor, as tensor_decompress_seg_each_dbatch takes them; all "pred": frames of tensor_compress_seg_pred_dbatch): the selection, the
        packed reader over the selected extents, the window fold, then planes_merge_window_each_dbatch.  Every other argument, the scratch,
        the workspace and the results are those of tensor_decompress_window_dbatch; the same segments are selected -- a pred window that
        starts inside a run of 1024 elements finds the differences in front of it in its first selected segment.  base (dst's layout, may
        be dst) is read for xor and sub tensors only; without one those are refused alone."""
        return _window_read(self, "tensor_decompress_window_each_dbatch", transforms, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log,
                            seg_first, n_segments, sel_first, n_selected, base, dst, dst_capacity, max_total_blocks, block_size_id, planes, planes_capacity,
                            sel_frame_offsets, sel_offsets, sel_results, plane_offsets, plane_sizes, workspace, results, 0)

    for f in (tensor_each_workspace_head, planes_split_each_dbatch, planes_merge_each_dbatch, tensor_compress_each_dbatch, tensor_compress_seg_each_dbatch,
              tensor_decompress_each_dbatch, tensor_decompress_seg_each_dbatch, planes_merge_window_each_dbatch, tensor_decompress_window_each_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- windows and patches of tensors with a stride per tensor (csrc/planes_each_stride_win.hip; fsehip.h, the section of that name): the four
    # window calls above and of "patching tensors with a transform per tensor" with `strides` behind `transforms`
    def planes_merge_window_each_stride_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, windows, elem_bytes, transforms, strides=None, base=None, dst=None,
                                               capacity=None, results=None):
        """planes_merge_window_each_dbatch with strides[i] (1 .. 8) the stride of tensor i where transforms[i] is pred: the lead is a % 1024
        elements at every stride, and all strides[i] chains are summed through it.  A 0 or a value above 8 there refuses that tensor alone
        (results -1, nothing of it read or written); for every other transform the entry is ignored.  strides: None (stride 1 everywhere:
        planes_merge_window_each_dbatch byte for byte), integers, or a CUDA uint8 tensor."""
        return planes_merge_window_each_dbatch(self, planes, plane_offsets, plane_sizes, dst_offsets, windows, elem_bytes, transforms, base, dst, capacity, results,
                                               _strides_arg=strides)

    def tensor_decompress_window_each_stride_dbatch(self, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes, segment_log, transforms, strides=None,
                                                    seg_first=None, n_segments=None, sel_first=None, n_selected=None, base=None, dst=None, dst_capacity=None,
                                                    max_total_blocks=None, block_size_id=5, planes=None, planes_capacity=None, sel_frame_offsets=None, sel_offsets=None,
                                                    sel_results=None, plane_offsets=None, plane_sizes=None, workspace=None, results=None):
        """tensor_decompress_window_each_dbatch for frames that tensor_compress_seg_each_stride_dbatch wrote with these transforms and strides
        (all "pred" and one stride: frames of tensor_compress_seg_pred_stride_dbatch): the same selection, reader and fold, then
        planes_merge_window_each_stride_dbatch.  strides None: tensor_decompress_window_each_dbatch byte for byte."""
        return _window_read(self, "tensor_decompress_window_each_stride_dbatch", transforms, frames, frame_offsets, src_offsets, windows, dst_offsets, elem_bytes,
                            segment_log, seg_first, n_segments, sel_first, n_selected, base, dst, dst_capacity, max_total_blocks, block_size_id, planes, planes_capacity,
                            sel_frame_offsets, sel_offsets, sel_results, plane_offsets, plane_sizes, workspace, results, 0, True, strides)

    def planes_split_window_each_stride_dbatch(self, src, src_offsets, windows, elem_bytes, segment_log, transforms, strides=None, stage_offsets=None, base=None,
                                               capacity=None, stage=None, stage_capacity=None, plane_offsets=None, results=None):
        """planes_split_window_each_dbatch with strides[i] (1 .. 8) the stride of tensor i where transforms[i] is pred: segments k0 .. k1 of the
        planes planes_split_each_stride_dbatch writes for the whole tensor -- a segment starts a run for every chain, so nothing in front of
        the staged bytes is read.  A 0 or a value above 8 there refuses that tensor alone (results -1, all its plane offsets its stage
        offset).  strides None: planes_split_window_each_dbatch byte for byte."""
        return _split_window(self, "planes_split_window_each_stride_dbatch", transforms, src, src_offsets, windows, elem_bytes, segment_log, stage_offsets, base, capacity,
                             stage, stage_capacity, plane_offsets, results, 0, True, strides)

    def tensor_patch_window_each_stride_dbatch(self, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes, segment_log, transforms, strides=None,
                                               seg_first=None, n_segments=None, sel_first=None, n_selected=None, stage_offsets=None, base=None, codec=0, codecs=None,
                                               new_codecs=None, block_size_id=5, capacity=None, frames_capacity=None, max_total_blocks=None, align_log=0, out=None,
                                               out_capacity=None, out_offsets=None, out_results=None, out_codecs=None, tensor_results=None, stage=None,
                                               stage_capacity=None, stage_plane_offsets=None, stage_seg_offsets=None, stage_results=None, new_frames=None,
                                               new_capacity=None, new_offsets=None, new_results=None, scratch=None, workspace=None):
        """tensor_patch_window_each_dbatch for an object that tensor_compress_seg_each_stride_dbatch wrote with these transforms and strides:
        planes_split_window_each_stride_dbatch, then the segments kernel, the packed writer and the splice as they are.  For tensors that differ
        inside the windows only, the result is tensor_compress_seg_each_stride_dbatch of src with the same transforms and strides given, byte
        for byte.  Both are GIVEN: the patch never chooses.  A pred tensor whose stride is 0 or above 8 is refused alone (-1) and keeps all
        its old frames.  strides None: tensor_patch_window_each_dbatch byte for byte."""
        return _patch_window(self, "tensor_patch_window_each_stride_dbatch", transforms, frames, frame_offsets, frame_results, src, src_offsets, windows, elem_bytes,
                             segment_log, seg_first, n_segments, sel_first, n_selected, stage_offsets, base, codec, codecs, new_codecs, block_size_id, capacity,
                             frames_capacity, max_total_blocks, align_log, out, out_capacity, out_offsets, out_results, out_codecs, tensor_results, stage, stage_capacity,
                             stage_plane_offsets, stage_seg_offsets, stage_results, new_frames, new_capacity, new_offsets, new_results, scratch, workspace, 0, True, strides)

    for f in (planes_merge_window_each_stride_dbatch, tensor_decompress_window_each_stride_dbatch, planes_split_window_each_stride_dbatch,
              tensor_patch_window_each_stride_dbatch):
        setattr(FseHip, f.__name__, f)

    # ---- tensor archives (csrc/planes_archive.hip; fsehip.h "tensor archives"): head | frames in one device buffer, sealed behind the frames a
    # compress call wrote at archive[head_bytes:], opened into the arrays the reading calls take
    def archive_head_bytes(self, n_tensors, n_frames, flags=0, meta_bytes=0):
        """the size of an archive's head for these counts (a multiple of 256): the frames start there.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_archive_headBytes.restype = SZ
        r = int(self.lib.FSEHIP_archive_headBytes(C.c_uint64(int(n_tensors)), C.c_uint64(int(n_frames)), C.c_uint(int(flags)), C.c_uint64(int(meta_bytes))))
        if r >= (1 << 62):
            raise ValueError("archive_head_bytes(%r, %r, %r, %r)" % (n_tensors, n_frames, flags, meta_bytes))
        return r

    def archive_info(self, elem_bytes, n_tensors, n_frames, total_bytes, flags=0, block_size_id=5, segment_log=0, delta_op=0, sparse_permille=0, max_total_blocks=0,
                     meta_bytes=0):
        """the ArchiveInfo a sender hands to archive_seal_dbatch, with head_bytes filled in (framesBytes is the device's to say)"""
        info = ArchiveInfo(ARCHIVE_MAGIC, ARCHIVE_VERSION, int(flags), _elem(elem_bytes), int(block_size_id), int(segment_log or 0), _delta_op(delta_op),
                           int(sparse_permille or 0), 0, int(n_tensors), int(n_frames), int(total_bytes), int(max_total_blocks), int(meta_bytes), 0, 0)
        info.headBytes = archive_head_bytes(self, n_tensors, n_frames, flags, meta_bytes)
        return info

    def archive_inspect(self, header, archive_bytes):
        """FSEHIP_archive_inspect: the first 64 bytes of an archive (host bytes / numpy) and the archive's size -> its ArchiveInfo; ValueError
        with the library's error name and the fields as read where a header rule refuses it.  Needs no device."""
        raw = np.frombuffer(bytes(header), dtype=np.uint8) if not isinstance(header, np.ndarray) else np.ascontiguousarray(header, dtype=np.uint8)
        if raw.size < 64:
            raise ValueError("archive_inspect: %d bytes, the header has 64" % raw.size)
        info = ArchiveInfo()
        self.lib.FSEHIP_archive_inspect.restype = SZ
        r = int(self.lib.FSEHIP_archive_inspect(C.byref(info), VP(raw.ctypes.data), C.c_uint64(int(archive_bytes))))
        if r >= (1 << 62):
            raise ValueError("archive header refused (%s) in %d bytes: %s" % (ERROR_NAMES.get((1 << 64) - r, "?"), archive_bytes,
                                                                              ", ".join("%s=%d" % (k, getattr(info, k)) for k, _ in ArchiveInfo._fields_)))
        return info

    def archive_workspace_bound(self, n_tensors, n_frames, head_bytes):
        """the workspace of archive_seal_dbatch and archive_open_dbatch.  Host arithmetic: needs no device."""
        self.lib.FSEHIP_archive_workspaceBound.restype = SZ
        r = int(self.lib.FSEHIP_archive_workspaceBound(C.c_uint64(int(n_tensors)), C.c_uint64(int(n_frames)), C.c_uint64(int(head_bytes))))
        if r >= (1 << 62):
            raise ValueError("archive_workspace_bound(%r, %r, %r)" % (n_tensors, n_frames, head_bytes))
        return r

    def _archive_ws(self, workspace, info, device):
        if workspace is None:
            return torch.empty(archive_workspace_bound(self, info.nTensors, info.nFrames, info.headBytes), dtype=torch.uint8, device=device)
        return self._flat(workspace, "workspace")

    def archive_seal_dbatch(self, archive, info, src_offsets, frame_offsets, frame_results, tensor_results, codecs=None, digests=None, meta=None, capacity=None,
                            result=None, workspace=None):
        """-> result (a CUDA int64 tensor of one entry: the archive's size head_bytes + framesBytes, or -2 where only the capacity was short and
        -1 for any other refusal -- the magic is then 0): writes the head of `archive` (a flat CUDA uint8 tensor) in front of the frames that a
        compress call wrote to archive[info.headBytes:].  src_offsets, frame_offsets, frame_results and tensor_results are that call's arrays
        as they are; codecs (uint8, with ARCHIVE_CODECS), digests (int64 bits, with ARCHIVE_DIGESTS) and meta (a CUDA uint8 tensor of
        info.metaBytes) as the flags say.  With src_offsets on the device, result and workspace given the call is launches only."""
        self._flat(archive, "archive")
        capacity = _room(self, archive, capacity, "archive")
        device = archive.device
        soff, _ = self._offsets(src_offsets, device, False)
        foff, _ = self._offsets(frame_offsets, device, False)
        nT, nF = int(info.nTensors), int(info.nFrames)
        if soff.numel() < nT + 1 or foff.numel() < nF + 1:
            raise ValueError("archive_seal_dbatch: %d source and %d frame offsets for %d tensors and %d frames" % (soff.numel(), foff.numel(), nT, nF))
        for what, t, n in (("frame_results", frame_results, nF), ("tensor_results", tensor_results, nT)):
            if t is None and n:
                raise ValueError("archive_seal_dbatch: %s of the compress call are needed" % what)
        res = _i64(self, result, 1, device, "result")
        fres = _i64(self, _some(frame_results), nF, device, "frame_results") if nF else res      # (an array of no entries still needs an address)
        tres = _i64(self, _some(tensor_results), nT, device, "tensor_results") if nT else res
        if info.flags & ARCHIVE_CODECS:
            codecs = _u8(_some(codecs), nF, device, "codecs")
        if info.flags & ARCHIVE_DIGESTS:
            if not isinstance(digests, torch.Tensor):
                digests = torch.from_numpy(np.asarray([int(d) & 0xFFFFFFFFFFFFFFFF for d in digests], dtype=np.uint64).astype(np.int64)).to(device)
            digests = _i64(self, _some(digests), nT, device, "digests")
        if info.metaBytes:
            meta = _u8(meta, int(info.metaBytes), device, "meta")
        workspace = _archive_ws(self, workspace, info, device)
        _check(self.lib.FSEHIP_archive_seal_dbatch(_ptr(archive), C.c_uint64(capacity), _ptr(res), C.byref(info), _ptr(soff), _ptr(foff), _ptr(fres), _ptr(tres),
                                                   _ptr(codecs if info.flags & ARCHIVE_CODECS else None), _ptr(digests if info.flags & ARCHIVE_DIGESTS else None),
                                                   _ptr(meta if info.metaBytes else None), _ptr(workspace), SZ(workspace.numel()), _stream()), "archive_seal_dbatch")
        return res

    def archive_open_dbatch(self, archive, info, archive_bytes=None, src_offsets=None, frame_offsets=None, codecs=None, digests=None, seg_first=None, verdict=None,
                            workspace=None):
        """-> dict(verdict, src_offsets, frame_offsets, codecs, digests, seg_first): the arrays of the archive at the start of `archive` (a flat
        CUDA uint8 tensor; `info` from archive_inspect of its first 64 bytes) as the reading calls take them, with frames =
        archive[info.headBytes:].  verdict (one int64 entry): the archive's size, or -4 -- then EVERY frame offset is 0 and every reader refuses
        every frame.  codecs / digests / seg_first are None where the archive has none.  With the outputs and the workspace given the call is
        launches only."""
        self._flat(archive, "archive")
        nbytes = _room(self, archive, archive_bytes, "archive")
        device = archive.device
        nT, nF, E = int(info.nTensors), int(info.nFrames), int(info.elemBytes)
        soff = _i64(self, src_offsets, nT + 1, device, "src_offsets")
        foff = _i64(self, frame_offsets, nF + 1, device, "frame_offsets")
        cod = dig = first = None
        if info.flags & ARCHIVE_CODECS:
            cod = torch.zeros(max(nF, 1), dtype=torch.uint8, device=device) if codecs is None else _u8(codecs, nF, device, "codecs")
        if info.flags & ARCHIVE_DIGESTS:
            dig = _i64(self, digests if digests is not None or nT else torch.zeros(1, dtype=torch.int64, device=device), nT, device, "digests")
        if info.segLog:
            first = _i64(self, seg_first, nT * E + 1, device, "seg_first")
        ver = _i64(self, verdict, 1, device, "verdict")
        workspace = _archive_ws(self, workspace, info, device)
        _check(self.lib.FSEHIP_archive_open_dbatch(_ptr(soff), _ptr(foff), _ptr(cod), _ptr(dig), _ptr(first), _ptr(ver), _ptr(archive), C.c_uint64(nbytes), C.byref(info),
                                                   _ptr(workspace), SZ(workspace.numel()), _stream()), "archive_open_dbatch")
        return dict(verdict=ver, src_offsets=soff, frame_offsets=foff, codecs=None if cod is None else cod[:nF], digests=None if dig is None else dig[:nT],
                    seg_first=first)

    def _codec_to_json(codec):
        if isinstance(codec, SparsePlanes):
            return {"sparse": _codec_to_json(codec.codec), "permille": codec.permille}
        if isinstance(codec, PredictedPlanes):
            j = {"pred": _codec_to_json(codec.codec)}
            if codec.stride != 1:
                j["stride"] = codec.stride
            return j
        if isinstance(codec, AutoCodec):
            return {"auto": codec.tolerance_permille}
        return int(codec)

    def _codec_from_json(j):
        if isinstance(j, dict) and "sparse" in j:
            return SparsePlanes(_codec_from_json(j["sparse"]), j["permille"])
        if isinstance(j, dict) and "pred" in j:
            return PredictedPlanes(_codec_from_json(j["pred"]), j.get("stride", 1))
        if isinstance(j, dict) and "auto" in j:
            return AutoCodec(j["auto"])
        return int(j)

    def _archive_meta(obj, gi, n_groups, idx, device_index, codec):
        """the meta record of group gi of `obj`, whose tensors are idx: what C has no notion of.  codec: the object's, as _codec_to_json gives it"""
        fields = dict(v=1, group=gi, groups=n_groups, tensors=len(obj.dtypes), index=idx, dtypes=[str(obj.dtypes[i]).replace("torch.", "") for i in idx],
                      shapes=[list(obj.shapes[i]) for i in idx], codec=codec, device_index=device_index)
        if getattr(obj, "transforms", None) is not None:        # compress_tensors_each's: the names travel as the predictor does
            fields["transforms"] = [obj.transforms[i] for i in idx]
            if any(st != 1 for st in (getattr(obj, "strides", None) or ())):      # (only where one exceeds 1: every other object's meta bytes stay as they were)
                fields["strides"] = [int(obj.strides[i]) for i in idx]
        return fields

    FseHip._archive_meta = staticmethod(_archive_meta)

    def archive_tensors(self, obj):
        """a CompressedTensors -> ONE flat CUDA uint8 tensor that holds all of it (include/fsehip.h "tensor archives"): one archive per group of
        obj.groups back to back, each at a multiple of 256 (an object without groups: one archive of no tensors), ready to be sent or written
        as it lies; open_archive restores the object from it.  A group's head carries its sizes, frame offsets, codecs, the digests of
        its bases and the scalars (element size, block_size_id, segment_log, delta_op, sparse_permille, the block promise); what C has no
        notion of -- the group's tensor indices, the dtypes and shapes, the number of groups and of tensors, obj.codec -- travels as JSON in
        the head's meta bytes.  THE FRAMES ARE COPIED HERE, device to device, behind their head: the object owns its frames elsewhere.  The
        path without a copy is the C one, where the compress call writes at d_archive + headBytes (archive_head_bytes, archive_seal_dbatch).
        One read-back per group (the seal's result); RuntimeError where the device refuses to seal."""
        if not isinstance(obj, CompressedTensors):
            raise TypeError("archive_tensors takes a CompressedTensors")
        device = obj.device if obj.device is not None else torch.device("cuda", torch.cuda.current_device())
        seg, sparse, digs = getattr(obj, "segment_log", None), getattr(obj, "sparse_permille", None), getattr(obj, "base_digests", None)
        n_groups = len(obj.groups)
        parts = []
        for gi, g in enumerate(obj.groups or [None]):
            E, idx, sizes = (1, [], []) if g is None else (g["elem_bytes"], list(g["index"]), list(g["sizes"]))
            meta = json.dumps(_archive_meta(obj, gi, n_groups, idx, device.index, _codec_to_json(obj.codec)), separators=(",", ":")).encode()
            flags = (ARCHIVE_DELTA if obj.delta else 0) | (ARCHIVE_SPARSE if sparse is not None else 0)
            flags |= (ARCHIVE_CODECS if g is not None and "codecs" in g else 0) | (ARCHIVE_DIGESTS if digs is not None and obj.delta else 0)
            nF = 0 if g is None else g["frame_offsets"].numel() - 1
            info = archive_info(self, E, len(sizes), nF, sum(sizes), flags, obj.block_size_id, seg or 0, getattr(obj, "delta_op", "xor") if obj.delta else 0,
                                sparse or 0, self.planes_block_bound(sum(sizes), len(sizes), E, obj.block_size_id), len(meta))
            head = int(info.headBytes)
            fb = 0 if g is None else int(g["frames"].numel())
            with torch.cuda.device(device):
                buf = torch.zeros((head + fb + 255) // 256 * 256, dtype=torch.uint8, device=device)
                if fb:
                    buf[head:head + fb] = g["frames"]
                zero = torch.zeros(1, dtype=torch.int64, device=device)
                res = archive_seal_dbatch(self, buf, info, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), zero if g is None else g["frame_offsets"],
                                          None if g is None else g["frame_results"], None if g is None else g["tensor_results"],
                                          codecs=g["codecs"] if flags & ARCHIVE_CODECS else None,
                                          digests=[digs[i] for i in idx] if flags & ARCHIVE_DIGESTS else None,
                                          meta=torch.from_numpy(np.frombuffer(meta, np.uint8).copy()).to(device), capacity=head + fb)
                got = int(res.item())
            if got != head + fb:
                raise RuntimeError("archive_tensors: group %d was not sealed (%d for %d bytes)" % (gi, got, head + fb))
            parts.append(buf)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def open_archive(self, buf):
        """what archive_tensors wrote -> the CompressedTensors: a flat CUDA uint8 tensor, or host bytes / a numpy uint8 array (uploaded to the
        current device).  The groups' frames are VIEWS into the buffer; segment_log, delta, delta_op, sparse_permille, base_digests, codec,
        dtypes and shapes are restored.  frame_results are the extents of the frame offsets and tensor_results the sizes: an archive exists
        only of frames that succeeded.  Per archive one 64-byte read-back for the header, FSEHIP_archive_open_dbatch, and one read-back of the
        verdict, the sizes and the meta bytes.  ValueError names what was refused: the header (with the library's error and the fields), the
        archive on the device (its digest, an index rule or a header that differs), or the meta bytes."""
        if not isinstance(buf, torch.Tensor):
            host = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
            buf = torch.from_numpy(host.copy()).cuda()
        self._flat(buf, "buf")
        device, total = buf.device, buf.numel()
        if total == 0:
            raise ValueError("open_archive: no bytes")
        groups, metas, at = [], [], 0
        with torch.cuda.device(device):
            while at < total:
                k = len(groups)
                if total - at < 64:
                    raise ValueError("open_archive: archive %d at byte %d: %d bytes, the header has 64" % (k, at, total - at))
                try:
                    info = archive_inspect(self, buf[at:at + 64].cpu().numpy(), total - at)
                except ValueError as e:
                    raise ValueError("open_archive: archive %d at byte %d: %s" % (k, at, e)) from None
                head, fb, nT, nF = int(info.headBytes), int(info.framesBytes), int(info.nTensors), int(info.nFrames)
                view = buf[at:at + head + fb]
                out = archive_open_dbatch(self, view, info)
                moff = 64 + 8 * nT + 8 * (nF + 1) + (8 * nT if info.flags & ARCHIVE_DIGESTS else 0) + ((nF + 7) // 8 * 8 if info.flags & ARCHIVE_CODECS else 0)
                got = torch.cat([out["verdict"], out["src_offsets"], out["digests"] if out["digests"] is not None else out["verdict"][:0]]).cpu().tolist()
                if got[0] != head + fb:
                    raise ValueError("open_archive: archive %d at byte %d was refused on the device (%s): its digest, an index rule or its header"
                                     % (k, at, ERROR_NAMES.get(-got[0], got[0])))
                try:
                    meta = json.loads(bytes(view[moff:moff + int(info.metaBytes)].cpu().numpy()).decode())
                    assert meta["v"] == 1 and meta["group"] == k and len(meta["index"]) == len(meta["dtypes"]) == len(meta["shapes"]) == nT
                    dtypes = [getattr(torch, d) for d in meta["dtypes"]]
                    assert all(isinstance(d, torch.dtype) for d in dtypes)
                    codec = _codec_from_json(meta["codec"])
                except Exception as e:
                    raise ValueError("open_archive: archive %d at byte %d: its meta bytes are not archive_tensors' (%s)" % (k, at, e)) from None
                S = got[1:nT + 2]
                g = dict(elem_bytes=int(info.elemBytes), index=[int(i) for i in meta["index"]], sizes=[b - a for a, b in zip(S, S[1:])], frames=view[head:head + fb],
                         frame_offsets=out["frame_offsets"], frame_results=out["frame_offsets"][1:] - out["frame_offsets"][:-1],
                         tensor_results=out["src_offsets"][1:] - out["src_offsets"][:-1])
                if out["codecs"] is not None:
                    g["codecs"] = out["codecs"]
                if out["seg_first"] is not None:
                    g["seg_first"] = out["seg_first"].cpu().numpy().astype(np.uint64)
                g["_info"], g["_meta"], g["_dtypes"], g["_codec"] = info, meta, dtypes, codec
                g["_digests"] = [d & 0xFFFFFFFFFFFFFFFF for d in got[nT + 2:]] if out["digests"] is not None else None
                groups.append(g)
                at += (head + fb + 255) // 256 * 256
                if len(groups) >= max(meta["groups"], 1):
                    break
        first, m0 = groups[0]["_info"], groups[0]["_meta"]
        n = int(m0["tensors"])
        if any(g["_meta"]["groups"] != m0["groups"] or g["_meta"]["tensors"] != n for g in groups) or len(groups) != max(m0["groups"], 1):
            raise ValueError("open_archive: %d archives of an object of %d groups" % (len(groups), m0["groups"]))
        dtypes, shapes = [None] * n, [None] * n
        digests = [None] * n if any(g["_digests"] is not None for g in groups) else None
        for g in groups:
            for k, i in enumerate(g["index"]):
                if not 0 <= i < n or dtypes[i] is not None:
                    raise ValueError("open_archive: tensor index %r of %d tensors" % (i, n))
                dtypes[i], shapes[i] = g["_dtypes"][k], tuple(int(x) for x in g["_meta"]["shapes"][k])
                if digests is not None:
                    digests[i] = g["_digests"][k]
        if any(d is None for d in dtypes):
            raise ValueError("open_archive: the archives hold %d of %d tensors" % (sum(d is not None for d in dtypes), n))
        delta = bool(first.flags & ARCHIVE_DELTA)
        codec = groups[0]["_codec"]
        transforms = None
        if any("transforms" in g["_meta"] for g in groups):
            transforms = [None] * n
            for g in groups:
                names = g["_meta"].get("transforms")
                if not isinstance(names, list) or len(names) != len(g["index"]) or any(t not in EST_NAMES for t in names):
                    raise ValueError("open_archive: the transforms in the meta bytes are not compress_tensors_each's (%r)" % (names,))
                for i, t in zip(g["index"], names):
                    transforms[i] = t
        strides = None
        if any("strides" in g["_meta"] for g in groups):
            strides = [1] * n
            for g in groups:
                sts = g["_meta"].get("strides")
                if (transforms is None or not isinstance(sts, list) or len(sts) != len(g["index"])
                        or any(isinstance(st, bool) or not isinstance(st, int) or not 1 <= st <= PRED_MAX_STRIDE for st in sts)):
                    raise ValueError("open_archive: the strides in the meta bytes are not compress_tensors_each's (%r)" % (sts,))
                for i, st in zip(g["index"], sts):
                    strides[i] = st
        for g in groups:
            for k in ("_info", "_meta", "_dtypes", "_codec", "_digests"):
                del g[k]
        obj = CompressedTensors(groups if m0["groups"] else [], dtypes, shapes, device if n else None, codec, int(first.blockSizeId), delta)
        if transforms is not None:
            obj.transforms = transforms
        if strides is not None:
            obj.strides = strides
        return _segmented(obj, int(first.segLog) if first.segLog else None, "sub" if delta and first.deltaOp else "xor",
                          int(first.sparsePermille) if first.flags & ARCHIVE_SPARSE else None, digests, codec.predictor if isinstance(codec, PredictedPlanes) else None)

    def save_tensors(self, obj, path):
        """archive_tensors(obj) written to the file `path` as it lies -> the number of bytes"""
        data = archive_tensors(self, obj).cpu().numpy()
        with open(path, "wb") as f:
            f.write(data.tobytes())
        return int(data.size)

    def load_tensors(self, path, device="cuda"):
        """open_archive of the file save_tensors wrote, uploaded to `device`"""
        with open(path, "rb") as f:
            data = np.frombuffer(f.read(), dtype=np.uint8)
        return open_archive(self, torch.from_numpy(data.copy()).to(device))

    for f in (archive_head_bytes, archive_info, archive_inspect, archive_workspace_bound, archive_seal_dbatch, archive_open_dbatch, archive_tensors, open_archive,
              save_tensors, load_tensors):
        setattr(FseHip, f.__name__, f)

    def _not_sparse(obj, what):
        if getattr(obj, "sparse_permille", None) is not None:
            raise ValueError(what + ": the object holds sparse planes (SparsePlanes); windows and patches of those are not supported")
        if getattr(obj, "predictor", None) is not None:
            raise ValueError(what + ": the object holds predicted planes (PredictedPlanes); decompress_tensor_windows_each reads windows of those, patches are not "
                             "supported")
        if getattr(obj, "transforms", None) is not None:
            raise ValueError(what + ": the object holds a transform per tensor (compress_tensors_each); decompress_tensor_windows_each reads windows of those, "
                             "patches are not supported")

    # ---- the user-facing pair
    def _read_base(obj, base, what):
        """the `base` of a reading call -> the plain sequence (or None) and the op of `obj`: a base iff the object holds deltas, and a
        DeltaBase only of the object's own op"""
        if getattr(obj, "delta", False) != (base is not None):
            raise ValueError(what + ": the object holds deltas and needs its base" if base is None else
                             what + ": the object holds no deltas, a base does not belong to it")
        op = getattr(obj, "delta_op", "xor")
        if isinstance(base, DeltaBase):
            if base.op != op:
                raise ValueError("%s: the base says op %r, the object was written with %r" % (what, base.op, op))
            base = base.tensors
        return base, _delta_op(op)

    def _bases(base, dtypes, shapes, device):
        """the `base` of the pair: one CUDA tensor per tensor, of its dtype, shape and device -> their bytes, flat"""
        base = list(base)
        if len(base) != len(dtypes):
            raise ValueError("base: %d tensors for %d" % (len(base), len(dtypes)))
        for k, (b, dt, sh) in enumerate(zip(base, dtypes, shapes)):
            if not isinstance(b, torch.Tensor) or not b.is_cuda or b.device != device or b.dtype != dt:
                raise TypeError("base[%d]: a CUDA tensor of %s on %s is needed" % (k, dt, device))
            if tuple(b.shape) != tuple(sh):
                raise ValueError("base[%d]: shape %s, the tensor's is %s" % (k, tuple(b.shape), tuple(sh)))
        return [b.contiguous().reshape(-1).view(torch.uint8) for b in base]

    def compress_tensors(self, tensors, codec=0, block_size_id=5, base=None):
        """CUDA tensors of any shapes and of dtypes of 1, 2, 4 or 8 bytes per element (TypeError otherwise) -> a CompressedTensors: every tensor as
        element-size .fse frames, one per byte plane.  Tensors are grouped by element_size(), one tensor_compress_dbatch per group; inputs that
        are not contiguous are made contiguous.  Reads the frames' total and results back once per group.  While a group is coded the call holds
        the concatenated inputs, a planes buffer of the same size and a frame buffer at frame_packed_bound -- about three to four times the
        group's bytes beside the inputs; the object keeps only the frames at their real total.
        base: a sequence of CUDA tensors matching `tensors` one to one in dtype, shape and device (TypeError / ValueError otherwise, before any
        launch) -- what the receiver already holds.  The frames then hold `tensor XOR base` (the object's `delta` is True), far fewer bytes where
        most bytes did not change, and decompress_tensors needs the same base.  A DeltaBase(tensors, "sub") as base: the frames hold
        zigzag(tensor - base) of the elements' bit patterns instead, fewer bytes again on weight updates; the object's `delta_op` is "sub"
        and the reading calls take the op from the object.
        codec: 0 (FSE), 1 (Huff0), an AutoCodec -- every plane's frame gets the codec chosen for it by size (tensor_compress_mixed_dbatch; each
        group dict gains "codecs", a CUDA uint8 tensor with entry i*E+p for plane p of the group's tensor i, and the object's `codec` is the
        AutoCodec) -- or a CompressedTensors an AutoCodec call returned for tensors of the same dtypes and shapes (ValueError otherwise, before
        any launch): its codecs are given again, nothing is tried twice.  An object compress_tensors_segmented wrote is refused here
        (ValueError): its codecs are per segment.  A SparsePlanes or a PredictedPlanes around 0, 1 or an AutoCodec: sparse contents, or the
        planes of the neighbour differences (the object's `predictor` is "prev", or "prev<S>" for PredictedPlanes(codec, stride=S), the
        predecessor S elements back for interleaved channels; ValueError with a base, before any launch).  For tensors
        above a few MiB use compress_tensors_segmented."""
        return _compress_tensors(self, tensors, codec, block_size_id, base, None)

    def compress_tensors_segmented(self, tensors, segment_log=18, codec=0, block_size_id=5, base=None):
        """compress_tensors with every plane cut into segments of 1 << segment_log bytes (10 + block_size_id .. 30, ValueError otherwise), one
        frame each (tensor_compress_seg_dbatch): the CompressedTensors has `segment_log` set, each group gains "seg_first", and frame_offsets,
        frame_results and codecs are per segment; decompress_tensors reads all of it from the object.  The frames hold the same blocks, eight
        bytes more per additional frame.  Why: a frame ends in one checksum over its whole content, a serial chain of about 1.5 GB/s per
        frame whatever else the device does, so a plane of hundreds of MiB as a single frame takes hundreds of milliseconds each way (one
        bf16 tensor of 1 GiB: 330 ms to write, 385 ms to read), while its segments run at the rate of as many small tensors (2.4 and 2.8 ms).
        Of 18, 20 and 22, 18 was the fastest on every shape measured, 20 within a quarter of it, 22 at half.  codec,
        block_size_id and base are compress_tensors'; an AutoCodec object given back as `codec` must have been written with the same
        segment_log (ValueError otherwise, before any launch)."""
        return _compress_tensors(self, tensors, codec, block_size_id, base,
                                 _seg_log(segment_log, block_size_id if isinstance(block_size_id, numbers.Integral) and 0 <= block_size_id <= 6 else 0))

    def _segmented(obj, segment_log, delta_op="xor", sparse=None, digests=None, predictor=None):
        if predictor is not None:
            obj.predictor = predictor
        if segment_log is not None:
            obj.segment_log = int(segment_log)
        if delta_op != "xor":
            obj.delta_op = delta_op
        if sparse is not None:
            obj.sparse_permille = int(sparse)
        if digests is not None:
            obj.base_digests = [int(d) for d in digests]
        return obj

    def _compress_tensors(self, tensors, codec, block_size_id, base, segment_log):
        tensors = list(tensors)
        earlier = None
        opname = "xor"
        digests = None
        if isinstance(base, DeltaBase):                     # the base with its op beside it; a plain sequence means XOR
            digests = [None] * len(tensors) if base.check else None
            base, opname = base.tensors, base.op
        op = _delta_op(opname)
        if isinstance(codec, CompressedTensors):            # the codecs an earlier AutoCodec call chose, given again
            earlier, codec = codec, codec.codec
            if getattr(earlier, "transforms", None) is not None:
                raise ValueError("compress_tensors: the earlier object holds a transform per tensor (compress_tensors_each), its codecs belong to those planes")
            if any("codecs" not in g for g in earlier.groups):
                raise ValueError("compress_tensors: the earlier object carries no codecs (it was not written with an AutoCodec)")
            if getattr(earlier, "segment_log", None) != segment_log:
                raise ValueError("compress_tensors: the earlier object was written with segment_log %r, this call has %r"
                                 % (getattr(earlier, "segment_log", None), segment_log))
            if len(earlier.dtypes) != len(tensors):
                raise ValueError("compress_tensors: the earlier object holds %d tensors, %d were given" % (len(earlier.dtypes), len(tensors)))
            for k, (t, dt, sh) in enumerate(zip(tensors, earlier.dtypes, earlier.shapes)):
                if isinstance(t, torch.Tensor) and (t.dtype != dt or tuple(t.shape) != tuple(sh)):
                    raise ValueError("compress_tensors: tensor %d is %s %s, the earlier object's was %s %s" % (k, t.dtype, tuple(t.shape), dt, tuple(sh)))
        sparse, outer = None, codec
        if isinstance(codec, SparsePlanes):                 # the contents' codec inside, the threshold beside it
            sparse, codec = codec.permille, codec.codec
        pred = None
        if isinstance(codec, PredictedPlanes):              # the planes' codec inside; the differences need no base and take none
            if base is not None:
                raise ValueError("compress_tensors: PredictedPlanes predicts from the tensor itself, a base does not go with it")
            pred, stride, codec = codec.predictor, codec.stride, codec.codec
        if not tensors:
            if base is not None and len(list(base)):
                raise ValueError("base: tensors for none")
            return _segmented(CompressedTensors([], [], [], None, outer, block_size_id, base is not None), segment_log, opname, sparse, digests, pred)
        device = tensors[0].device
        for t in tensors:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
                raise TypeError("compress_tensors takes CUDA tensors of one device")
            _elem(t.element_size())
        braw = None if base is None else _bases(base, [t.dtype for t in tensors], [tuple(t.shape) for t in tensors], device)
        groups = []
        for E in (1, 2, 4, 8):
            idx = [i for i, t in enumerate(tensors) if t.element_size() == E]
            if not idx:
                continue
            raw = [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx]
            offs = np.concatenate([[0], np.cumsum([r.numel() for r in raw])]).astype(np.uint64)
            src = torch.cat(raw) if int(offs[-1]) else torch.zeros(1, dtype=torch.uint8, device=device)[:0]
            bsrc = None if braw is None else torch.cat([braw[i] for i in idx]) if int(offs[-1]) else src
            codecs = sfirst = None
            if pred is not None:
                given = None if earlier is None else [g for g in earlier.groups if g["elem_bytes"] == E][0]["codecs"]
                if segment_log is not None:
                    sfirst = self.planes_segment_first(np.diff(offs.astype(np.int64)), E, segment_log)
                    if stride == 1:
                        dst, foff, fres, tres, codecs = self.tensor_compress_seg_pred_dbatch(src, offs, E, segment_log, sfirst, codec=codec, codecs=given,
                                                                                             block_size_id=block_size_id)
                    else:
                        dst, foff, fres, tres, codecs = self.tensor_compress_seg_pred_stride_dbatch(src, offs, E, stride, segment_log, sfirst, codec=codec,
                                                                                                    codecs=given, block_size_id=block_size_id)
                elif stride == 1:
                    dst, foff, fres, tres, codecs = self.tensor_compress_pred_dbatch(src, offs, E, codec=codec, codecs=given, block_size_id=block_size_id)
                else:
                    dst, foff, fres, tres, codecs = self.tensor_compress_pred_stride_dbatch(src, offs, E, stride, codec=codec, codecs=given,
                                                                                            block_size_id=block_size_id)
            elif sparse is not None:
                given = None if earlier is None else [g for g in earlier.groups if g["elem_bytes"] == E][0]["codecs"]
                if segment_log is not None:
                    sfirst = self.planes_segment_first(np.diff(offs.astype(np.int64)), E, segment_log)
                    dst, foff, fres, tres, codecs = self.tensor_compress_seg_sparse_dbatch(src, offs, E, segment_log, sparse, sfirst, base=bsrc, codec=codec,
                                                                                           codecs=given, block_size_id=block_size_id, delta_op=op)
                else:
                    dst, foff, fres, tres, codecs = self.tensor_compress_sparse_dbatch(src, offs, E, sparse, base=bsrc, codec=codec, codecs=given,
                                                                                       block_size_id=block_size_id, delta_op=op)
            elif segment_log is not None:
                given = None if earlier is None else [g for g in earlier.groups if g["elem_bytes"] == E][0]["codecs"]
                sfirst = self.planes_segment_first(np.diff(offs.astype(np.int64)), E, segment_log)
                dst, foff, fres, tres, codecs = self.tensor_compress_seg_dbatch(src, offs, E, segment_log, sfirst, base=bsrc, codec=codec, codecs=given,
                                                                                block_size_id=block_size_id, delta_op=op)
            elif isinstance(codec, AutoCodec):
                given = None if earlier is None else [g for g in earlier.groups if g["elem_bytes"] == E][0]["codecs"]
                dst, foff, fres, tres, codecs = self.tensor_compress_mixed_dbatch(src, offs, E, bsrc, given, codec.tolerance_permille, block_size_id, delta_op=op)
            elif braw is None:
                dst, foff, fres, tres = self.tensor_compress_dbatch(src, offs, E, block_size_id, codec)
            else:
                dst, foff, fres, tres = self.tensor_compress_delta_dbatch(src, bsrc, offs, E, block_size_id, codec, delta_op=op)
            got = torch.cat([foff[-1:], fres, tres]).cpu().tolist()
            if min(got) < 0:
                bad = [k for k, r in enumerate(got[1:1 + fres.numel()]) if r < 0]
                raise RuntimeError("compress_tensors: element size %d, frames %s failed (%s)" % (E, bad[:8], [got[1 + k] for k in bad[:8]]))
            groups.append(dict(elem_bytes=E, index=idx, sizes=[int(x) for x in np.diff(offs)], frames=dst[:got[0]].clone(), frame_offsets=foff,
                               frame_results=fres, tensor_results=tres))
            if codecs is not None:
                groups[-1]["codecs"] = codecs.clone()
            if sfirst is not None:
                groups[-1]["seg_first"] = sfirst
            if digests is not None:                         # the base's digests: what the receiver's base has to show
                for i, d in zip(idx, _group_digests(self, [braw[i] for i in idx], device, bsrc)):
                    digests[i] = d
        return _segmented(CompressedTensors(groups, [t.dtype for t in tensors], [tuple(t.shape) for t in tensors], device, outer, block_size_id, braw is not None),
                          segment_log, opname if braw is not None else "xor", sparse, digests, pred)

    def _base_copy(braw, g, device, held=None):
        """the bases of a group back to back, as the copy a group is rebuilt over in place (held: the one that was digested)"""
        if held is not None:
            return held
        return torch.cat([braw[i] for i in g["index"]]) if sum(g["sizes"]) else torch.zeros(1, dtype=torch.uint8, device=device)[:0]

    def _gate_groups(self, obj, braw):
        """decompress_tensors of an object with base_digests: per group the copy of the given bases, digested, and the gated frame offsets.
        ValueError naming the tensors whose base is not the one the object was written against -- before any decode launch"""
        expected = obj.base_digests
        if braw is None or len(expected) != len(obj.dtypes):
            raise ValueError("decompress_tensors: base_digests holds %d entries for %d tensors" % (len(expected), len(obj.dtypes)))
        checked, verdicts = [], []
        for g in obj.groups:
            E, idx = g["elem_bytes"], g["index"]
            offs = np.concatenate([[0], np.cumsum(g["sizes"])]).astype(np.uint64)
            held = _base_copy(braw, g, obj.device)
            dig, res = tensor_digest_dbatch(self, held, offs)
            gated, gres = tensor_gate_dbatch(self, g["frame_offsets"], dig, res, [expected[i] for i in idx], E, g.get("seg_first"))
            checked.append((held, gated))
            verdicts.append(gres)
        got = torch.cat(verdicts).cpu().tolist() if verdicts else []
        bad = sorted(i for i, r in zip([i for g in obj.groups for i in g["index"]], got) if r < 0)
        if bad:
            raise ValueError("decompress_tensors: the base of tensors %s is not the one the object was written against (its digest differs)" % (bad,))
        return checked

    def decompress_tensors(self, obj, base=None):
        """-> the tensors compress_tensors was given, in their order: same dtype, shape and device, the same bytes.  Every tensor owns its memory
        (a copy out of the group's destination buffer).  The block promise is planes_block_bound of the recorded sizes: no query, no read-back
        before the results.
        base: for an object with `delta` set, the tensors compress_tensors was given as base (checked for dtype, shape and device, not for
        content: the frames do not say what they are a delta against).  ValueError for a delta object without a base and for a base with a plain
        object.  The bases are not changed: a group is rebuilt in place over a copy of its bases.  The delta's op ("xor" or "sub") is the
        object's `delta_op`; the base is the plain sequence, or a DeltaBase of the same op (ValueError for another, before any launch).
        An object with `base_digests` (written against a DeltaBase(..., check=True)): the given base is digested and compared on the device
        (tensor_digest_dbatch, tensor_gate_dbatch; one read-back of the verdicts) and ValueError names the tensors whose base is not the one
        the deltas were made against -- before any decode launch, nothing is written; the readers then run over the gated offsets.
        A TensorBundle (compress_tensors_auto): every part is read as above and the tensors come back in the input order; `base` is the base
        of the WHOLE list, each delta part is handed its slice of it; ValueError before any launch where a delta part has no base.
        An object with `transforms` (compress_tensors_each): tensor_decompress_each_dbatch per group; `base` is the base of the whole list and
        is needed only where a tensor's transform is "xor" or "sub" (ValueError before any launch without it)."""
        if isinstance(obj, TensorBundle):                    # compress_tensors_auto's: part by part, each with its slice of the base
            return _decompress_bundle(self, obj, base)
        if getattr(obj, "transforms", None) is not None:     # compress_tensors_each's: one object, a transform per tensor
            return _decompress_each_obj(self, obj, base)
        base, op = _read_base(obj, base, "decompress_tensors")
        stride = None if getattr(obj, "predictor", None) is None else predictor_stride(obj.predictor, "decompress_tensors")
        braw = None if base is None else _bases(base, obj.dtypes, obj.shapes, obj.device)
        checked = _gate_groups(self, obj, braw) if getattr(obj, "base_digests", None) is not None else None
        out = [None] * len(obj.dtypes)
        for gi, g in enumerate(obj.groups):
            E, sizes = g["elem_bytes"], g["sizes"]
            offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            blocks = self.planes_block_bound(sum(sizes), len(sizes), E, obj.block_size_id)
            seg_log = getattr(obj, "segment_log", None)
            held, foff = checked[gi] if checked is not None else (None, g["frame_offsets"])     # (checked: the copy that was digested, the gated offsets)
            if stride == 1:
                if seg_log is not None:
                    dst, res = self.tensor_decompress_seg_pred_dbatch(g["frames"], foff, offs, E, seg_log, g["seg_first"], max_total_blocks=blocks)
                else:
                    dst, res = self.tensor_decompress_pred_dbatch(g["frames"], foff, offs, E, max_total_blocks=blocks)
            elif stride is not None:
                if seg_log is not None:
                    dst, res = self.tensor_decompress_seg_pred_stride_dbatch(g["frames"], foff, offs, E, stride, seg_log, g["seg_first"], max_total_blocks=blocks)
                else:
                    dst, res = self.tensor_decompress_pred_stride_dbatch(g["frames"], foff, offs, E, stride, max_total_blocks=blocks)
            elif getattr(obj, "sparse_permille", None) is not None:
                dst = None if braw is None else _base_copy(braw, g, obj.device, held)
                if seg_log is not None:
                    dst, res = self.tensor_decompress_seg_sparse_dbatch(g["frames"], foff, offs, E, seg_log, g["seg_first"], base=dst, dst=dst,
                                                                        max_total_blocks=blocks, delta_op=op)
                else:
                    dst, res = self.tensor_decompress_sparse_dbatch(g["frames"], foff, offs, E, base=dst, dst=dst, max_total_blocks=blocks, delta_op=op)
            elif seg_log is not None:
                dst = None if braw is None else _base_copy(braw, g, obj.device, held)
                dst, res = self.tensor_decompress_seg_dbatch(g["frames"], foff, offs, E, seg_log, g["seg_first"], base=dst, dst=dst,
                                                             max_total_blocks=blocks, delta_op=op)
            elif braw is None:
                dst, res = self.tensor_decompress_dbatch(g["frames"], foff, offs, E, max_total_blocks=blocks)
            else:
                dst = _base_copy(braw, g, obj.device, held)
                dst, res = self.tensor_decompress_delta_dbatch(g["frames"], foff, dst, offs, E, dst=dst, max_total_blocks=blocks, delta_op=op)
            got = res.cpu().tolist()
            if got != sizes:
                raise RuntimeError("decompress_tensors: element size %d, results %s for tensors of %s bytes" % (E, got[:8], sizes[:8]))
            for k, i in enumerate(g["index"]):
                out[i] = dst[int(offs[k]):int(offs[k + 1])].clone().view(obj.dtypes[i]).reshape(obj.shapes[i])
        return out

    def _margin(margin_permille, what):
        if not isinstance(margin_permille, numbers.Integral) or isinstance(margin_permille, bool) or not 0 <= margin_permille <= 1000:
            raise ValueError("%s: margin_permille %r, 0 .. 1000 is needed" % (what, margin_permille))
        return int(margin_permille)

    def estimate_tensors(self, tensors, base=None, candidates=None, margin_permille=50, strides=None):
        """CUDA tensors of one device and of 1, 2, 4 or 8 bytes per element -> one record per tensor, in input order: dict(bytes=its size,
        estimates={name: estimated bytes of its frames under that plane transform}, choice=name).  The names: "plain" (compress_tensors as
        it is), "pred" (PredictedPlanes), "xor" (base=...), "sub" (DeltaBase(..., "sub")).  One read of the tensors (and of the bases) on the
        device (planes_estimate_dbatch; fsehip.h "plane estimates": the order-0 cost of every candidate's planes in integers, no plane
        buffer, no coder), one call and one read-back per group of one element size; the tensors of a group are concatenated as
        compress_tensors does it.
        base: a sequence matching `tensors` one to one as compress_tensors takes it (or a DeltaBase: its tensors, the op is what is being
        chosen).  candidates: names out of the four, default ("plain", "pred") without a base and all four with one; "xor" and "sub" need
        a base.  The choice: the first candidate in the order above, replaced by a later one only if that is more than margin_permille /
        1000 smaller than the best so far -- hysteresis towards the simpler form, a policy like AutoCodec's tolerance.  An estimate has
        no term for frame headers or tables.  TypeError / ValueError as compress_tensors raises them, before any launch.
        strides: None, or a sequence of integers out of 1 .. 8, the strides at which "pred" is estimated (planes_estimate_stride_dbatch):
        the records gain stride=the stride chosen among them in rising order under the same margin, and stride_estimates={S: bytes};
        estimates["pred"] is the estimate at that stride.  "pred" must be among the candidates."""
        margin = _margin(margin_permille, "estimate_tensors")
        smask = None if strides is None else _stride_mask(strides, "estimate_tensors")
        tensors = list(tensors)
        if isinstance(base, DeltaBase):
            base = base.tensors
        if candidates is None:
            candidates = EST_NAMES[:2] if base is None else EST_NAMES
        if isinstance(candidates, str) or not len(candidates) or any(not isinstance(c, str) or c not in EST_NAMES for c in candidates):
            raise ValueError("estimate_tensors: candidates %r, names out of %r are needed" % (candidates, EST_NAMES))
        mask = 0
        for c in candidates:
            mask |= 1 << EST_NAMES.index(c)
        if (mask & 12) and base is None:
            raise ValueError("estimate_tensors: \"xor\" and \"sub\" are deltas against a base, none was given")
        if smask is not None and not mask & 2:
            raise ValueError("estimate_tensors: strides are candidates of \"pred\", which is not among the candidates %r" % (tuple(candidates),))
        if not tensors:
            if base is not None and len(list(base)):
                raise ValueError("base: tensors for none")
            return []
        device = tensors[0].device if isinstance(tensors[0], torch.Tensor) else None
        for k, t in enumerate(tensors):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
                raise TypeError("estimate_tensors takes CUDA tensors of one device")
            _elem(t.element_size())
            if t.numel() * t.element_size() >= 1 << 32:
                raise ValueError("estimate_tensors: tensor %d holds 2^32 bytes or more, the counts are 32 bits wide" % k)
        braw = None if base is None else _bases(base, [t.dtype for t in tensors], [tuple(t.shape) for t in tensors], device)
        out = [None] * len(tensors)
        with torch.cuda.device(device):
            for E in (1, 2, 4, 8):
                idx = [i for i, t in enumerate(tensors) if t.element_size() == E]
                if not idx:
                    continue
                raw = [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx]
                offs = np.concatenate([[0], np.cumsum([r.numel() for r in raw])]).astype(np.uint64)
                one = len(raw) == 1 and raw[0].numel() > 0          # a single tensor is estimated where it lies
                src = raw[0] if one else torch.cat(raw) if int(offs[-1]) else torch.zeros(1, dtype=torch.uint8, device=device)[:0]
                bsrc = None if braw is None or not (mask & 12) else braw[idx[0]] if one else torch.cat([braw[i] for i in idx]) if int(offs[-1]) else src
                n = len(idx)
                if smask is None:
                    _, eb, ch, res = planes_estimate_dbatch(self, src, offs, E, mask, margin, bsrc)
                    got = torch.cat([eb, ch.to(torch.int64), res]).cpu().tolist()
                else:
                    _, eb, ch, res, seb, st = planes_estimate_stride_dbatch(self, src, offs, E, mask, smask, margin, bsrc)
                    got = torch.cat([eb, ch.to(torch.int64), res, st.to(torch.int64), seb]).cpu().tolist()
                if got[5 * n:6 * n] != [int(x) for x in np.diff(offs.astype(np.int64))]:
                    raise RuntimeError("estimate_tensors: element size %d, results %s" % (E, got[5 * n:5 * n + 8]))
                for k, i in enumerate(idx):
                    out[i] = dict(bytes=got[5 * n + k], estimates={name: got[4 * k + c] for c, name in enumerate(EST_NAMES) if (mask >> c) & 1},
                                  choice=EST_NAMES[got[4 * n + k]])
                    if smask is not None:
                        out[i]["stride"] = got[6 * n + k]
                        out[i]["stride_estimates"] = {S: got[7 * n + 8 * k + S - 1] for S in range(1, PRED_MAX_STRIDE + 1) if (smask >> (S - 1)) & 1}
        return out

    def compress_tensors_auto(self, tensors, base=None, codec=0, block_size_id=5, segment_log=None, margin_permille=50):
        """A mixed list of CUDA tensors (a state_dict's values: weights, index buffers, position ids, masks, statistics) -> a TensorBundle:
        estimate_tensors chooses the plane transform per tensor, the list is cut by choice, and every non-empty part goes through the
        existing call once -- compress_tensors (or, with segment_log, compress_tensors_segmented) as it is, with PredictedPlanes(codec),
        with base= the part's bases, or with DeltaBase(the part's bases, "sub").  Without a base the candidates are "plain" and "pred", with
        one all four.  codec: 0, 1 or an AutoCodec -- the coder of every part; block_size_id, segment_log: the existing calls'.  The frames
        are ordinary frames: nothing in them records the choice, the bundle does.  decompress_tensors(bundle, base) gives the list back.
        A tensor of 0 bytes (every estimate 0) is filed with the first part that holds bytes of its element size -- the frame writers take
        no group of no bytes -- and its record's choice says so."""
        margin = _margin(margin_permille, "compress_tensors_auto")
        pred = PredictedPlanes(codec)                          # (0, 1 or an AutoCodec, or ValueError -- whether or not a tensor will want it)
        if segment_log is not None:
            segment_log = _seg_log(segment_log, block_size_id if isinstance(block_size_id, numbers.Integral) and 0 <= block_size_id <= 6 else 0)
        tensors = list(tensors)
        if isinstance(base, DeltaBase):
            base = base.tensors
        base = None if base is None else list(base)
        records = estimate_tensors(self, tensors, base, None, margin)
        for i, r in enumerate(records):                        # a tensor of no bytes has nothing to choose: it goes where its element size has company
            if r["bytes"] == 0:
                held = [q["choice"] for t, q in zip(tensors, records) if q["bytes"] and t.element_size() == tensors[i].element_size()]
                r["choice"] = next((name for name in EST_NAMES if name in held), r["choice"])

        def part(sub, codec, base):
            if segment_log is None:
                return compress_tensors(self, sub, codec, block_size_id, base)
            return compress_tensors_segmented(self, sub, segment_log, codec, block_size_id, base)
        parts, index = {}, {}
        for name in EST_NAMES:
            idx = [i for i, r in enumerate(records) if r["choice"] == name]
            if not idx:
                continue
            sub = [tensors[i] for i in idx]
            index[name] = idx
            if name == "plain":
                parts[name] = part(sub, codec, None)
            elif name == "pred":
                parts[name] = part(sub, pred, None)
            elif name == "xor":
                parts[name] = part(sub, codec, [base[i] for i in idx])
            else:
                parts[name] = part(sub, codec, DeltaBase([base[i] for i in idx], "sub"))
        return TensorBundle(parts, index, records, len(tensors))

    def _decompress_bundle(self, bundle, base):
        if isinstance(base, DeltaBase):
            base = base.tensors
        base = None if base is None else list(base)
        n = bundle.n_tensors
        if sorted(i for idx in bundle.index.values() for i in idx) != list(range(n)) or set(bundle.index) != set(bundle.parts) or not set(bundle.parts) <= set(EST_NAMES):
            raise ValueError("decompress_tensors: the bundle's parts do not partition its %d tensors" % n)
        if base is None and any(name in ("xor", "sub") for name in bundle.parts):
            raise ValueError("decompress_tensors: the bundle holds deltas and needs its base")
        if base is not None and len(base) != n:
            raise ValueError("base: %d tensors for %d" % (len(base), n))
        out = [None] * n
        for name in EST_NAMES:
            if name not in bundle.parts:
                continue
            idx = bundle.index[name]
            back = decompress_tensors(self, bundle.parts[name], [base[i] for i in idx] if name in ("xor", "sub") else None)
            for i, t in zip(idx, back):
                out[i] = t
        return out

    def compress_tensors_each(self, tensors, transforms="auto", base=None, codec=0, block_size_id=5, segment_log=None, margin_permille=50, strides=None):
        """A mixed list of CUDA tensors -> ONE CompressedTensors whose `transforms` lists the plane transform of every tensor ("plain", "pred",
        "xor", "sub"): what compress_tensors_auto chooses, without cutting the list -- per group of one element size one
        tensor_compress_each_dbatch (with segment_log: tensor_compress_seg_each_dbatch), which estimates, chooses, splits and writes on the
        device, and ONE read-back at the end: the frame total, the results and the choices.  The object is an ordinary one: archive_tensors,
        open_archive, save_tensors and load_tensors carry it (the names travel in the meta bytes), decompress_tensors(obj, base) reads it.
        transforms: "auto" -- the candidates are "plain" and "pred" without a base and all four with one, margin_permille as
        estimate_tensors takes it -- or one name per tensor, given ("choose once, then give": obj.transforms of an earlier call).
        base: a sequence matching `tensors` one to one (or a DeltaBase without check: its tensors); needed where a given name is "xor" or
        "sub".  codec: 0, 1 or an AutoCodec.  A tensor of 0 bytes takes the lowest candidate and needs no company.
        strides: None -- "pred" is stride 1, as ever -- or, with "auto", the candidate strides of "pred" (integers out of 1 .. 8: the stride of
        every tensor is chosen with its transform, interleaved channels find their channel count), or, with given names, one stride per
        tensor (obj.strides of an earlier call; looked at for the "pred" ones).  The object's `strides` lists the stride of every tensor, 1
        for those that are not "pred"; archives and files carry it where one exceeds 1.
        Out of scope, each a ValueError before any launch: a SparsePlanes or PredictedPlanes as codec, an earlier object as codec, a
        DeltaBase(check=True); a stride outside 1 .. 8; strides with "auto" where "pred" is no candidate.  Windows of a segmented object are read by
        decompress_tensor_windows_each and written by patch_tensor_windows_each, not by decompress_tensor_windows and patch_tensor_windows; those
        of an object with a stride above 1 by decompress_tensor_windows_each_stride and patch_tensor_windows_each_stride alone."""
        what = "compress_tensors_each"
        margin = _margin(margin_permille, what)
        if isinstance(codec, bool) or not (isinstance(codec, AutoCodec) or (isinstance(codec, numbers.Integral) and codec in (0, 1))):
            raise ValueError("%s: codec %r; 0, 1 or an AutoCodec is needed (sparse planes, predicted planes and earlier objects do not go around a transform per "
                             "tensor)" % (what, codec))
        if isinstance(base, DeltaBase):
            if base.check:
                raise ValueError(what + ": DeltaBase(check=True) -- digests and gating are not supported with a transform per tensor")
            base = base.tensors
        base = None if base is None else list(base)
        if segment_log is not None:
            segment_log = _seg_log(segment_log, block_size_id if isinstance(block_size_id, numbers.Integral) and 0 <= block_size_id <= 6 else 0)
        tensors = list(tensors)
        auto = isinstance(transforms, str)
        if auto and transforms != "auto":
            raise ValueError("%s: transforms %r; \"auto\" or one name per tensor out of %r is needed" % (what, transforms, EST_NAMES))
        if not auto:
            transforms = list(transforms)
            if len(transforms) != len(tensors) or any(not isinstance(t, str) or t not in EST_NAMES for t in transforms):
                raise ValueError("%s: transforms %r; \"auto\" or one name per tensor (%d) out of %r is needed" % (what, transforms[:8], len(tensors), EST_NAMES))
            if base is None and any(t in ("xor", "sub") for t in transforms):
                raise ValueError(what + ": \"xor\" and \"sub\" are deltas against a base, none was given")
        smask = None
        if strides is not None and auto:
            smask = _stride_mask(list(strides), what)             # ("pred" is a candidate of every "auto" call)
        elif strides is not None:
            strides = list(strides)
            if len(strides) != len(tensors):
                raise ValueError("%s: %d strides for %d tensors" % (what, len(strides), len(tensors)))
            for st in strides:
                _stride(st, what)
            strides = [int(st) if t == "pred" else 1 for st, t in zip(strides, transforms)]
        if not tensors:
            if base is not None and len(base):
                raise ValueError("base: tensors for none")
            obj = _segmented(CompressedTensors([], [], [], None, codec, block_size_id), segment_log)
            obj.transforms = []
            if strides is not None:
                obj.strides = []
            return obj
        device = tensors[0].device if isinstance(tensors[0], torch.Tensor) else None
        for k, t in enumerate(tensors):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
                raise TypeError(what + " takes CUDA tensors of one device")
            _elem(t.element_size())
            if auto and t.numel() * t.element_size() >= 1 << 32:
                raise ValueError("%s: tensor %d holds 2^32 bytes or more, the estimate's counts are 32 bits wide" % (what, k))
        braw = None if base is None else _bases(base, [t.dtype for t in tensors], [tuple(t.shape) for t in tensors], device)
        names, groups, chosen = [None] * len(tensors), [], [1] * len(tensors)
        with torch.cuda.device(device):
            for E in (1, 2, 4, 8):
                idx = [i for i, t in enumerate(tensors) if t.element_size() == E]
                if not idx:
                    continue
                raw = [tensors[i].contiguous().reshape(-1).view(torch.uint8) for i in idx]
                offs = np.concatenate([[0], np.cumsum([r.numel() for r in raw])]).astype(np.uint64)
                src = torch.cat(raw) if int(offs[-1]) else torch.zeros(1, dtype=torch.uint8, device=device)[:0]
                bsrc = None if braw is None else torch.cat([braw[i] for i in idx]) if int(offs[-1]) else src
                given = None if auto else [transforms[i] for i in idx]
                sfirst = None
                st = None
                if segment_log is not None:
                    sfirst = self.planes_segment_first(np.diff(offs.astype(np.int64)), E, segment_log)
                if strides is not None:                         # the calls with a stride per tensor: given with the names, or chosen with them
                    gs = None if auto else [strides[i] for i in idx]
                    if segment_log is not None:
                        dst, foff, fres, tres, codecs, tr, st = tensor_compress_seg_each_stride_dbatch(self, src, offs, E, segment_log, given, gs, bsrc, None, smask, margin,
                                                                                                       seg_first=sfirst, codec=codec, block_size_id=block_size_id)
                    else:
                        dst, foff, fres, tres, codecs, tr, st = tensor_compress_each_stride_dbatch(self, src, offs, E, given, gs, bsrc, None, smask, margin, codec=codec,
                                                                                                   block_size_id=block_size_id)
                elif segment_log is not None:
                    dst, foff, fres, tres, codecs, tr = tensor_compress_seg_each_dbatch(self, src, offs, E, segment_log, given, bsrc, None, margin, seg_first=sfirst,
                                                                                        codec=codec, block_size_id=block_size_id)
                else:
                    dst, foff, fres, tres, codecs, tr = tensor_compress_each_dbatch(self, src, offs, E, given, bsrc, None, margin, codec=codec, block_size_id=block_size_id)
                nf, n = fres.numel(), len(idx)
                got = torch.cat([foff[-1:], fres, tres, tr.to(torch.int64)] + ([] if st is None else [st.to(torch.int64)])).cpu().tolist()      # the one read-back of the group
                if st is not None:
                    got, gst = got[:1 + nf + 2 * n], got[1 + nf + 2 * n:]
                    if any(not 1 <= x <= PRED_MAX_STRIDE for x in gst):
                        raise RuntimeError("%s: element size %d, strides %s" % (what, E, gst[:8]))
                    for k, i in enumerate(idx):
                        chosen[i] = gst[k]
                if min(got[:1 + nf + n]) < 0 or max(got[1 + nf + n:]) > 3:
                    bad = [k for k, r in enumerate(got[1:1 + nf]) if r < 0]
                    raise RuntimeError("%s: element size %d, frames %s failed (%s), tensor results %s, transforms %s"
                                       % (what, E, bad[:8], [got[1 + k] for k in bad[:8]], got[1 + nf:1 + nf + n][:8], got[1 + nf + n:][:8]))
                for k, i in enumerate(idx):
                    names[i] = EST_NAMES[got[1 + nf + n + k]]
                groups.append(dict(elem_bytes=E, index=idx, sizes=[int(x) for x in np.diff(offs)], frames=dst[:got[0]].clone(), frame_offsets=foff,
                                   frame_results=fres, tensor_results=tres))
                if codecs is not None:
                    groups[-1]["codecs"] = codecs.clone()
                if sfirst is not None:
                    groups[-1]["seg_first"] = sfirst
        obj = _segmented(CompressedTensors(groups, [t.dtype for t in tensors], [tuple(t.shape) for t in tensors], device, codec, block_size_id), segment_log)
        obj.transforms = names
        if strides is not None:
            obj.strides = chosen
        return obj

    def _obj_strides(obj, what):
        """the strides of an object with a transform per tensor: None (stride 1 everywhere), or one integer 1 .. 8 per tensor"""
        strides = getattr(obj, "strides", None)
        if strides is None:
            return None
        strides = list(strides)
        if len(strides) != len(obj.dtypes):
            raise ValueError("%s: %d strides for %d tensors" % (what, len(strides), len(obj.dtypes)))
        for st in strides:
            _stride(st, what)
        return [int(st) for st in strides]

    def _decompress_each_obj(self, obj, base):
        what = "decompress_tensors"
        names = list(obj.transforms)
        if len(names) != len(obj.dtypes) or any(t not in EST_NAMES for t in names):
            raise ValueError("%s: transforms %r; one name per tensor (%d) out of %r is needed" % (what, names[:8], len(obj.dtypes), EST_NAMES))
        if getattr(obj, "sparse_permille", None) is not None or getattr(obj, "base_digests", None) is not None or getattr(obj, "predictor", None) is not None:
            raise ValueError(what + ": sparse planes, base digests and a predictor do not go with a transform per tensor")
        strides = _obj_strides(obj, what)
        if isinstance(base, DeltaBase):
            base = base.tensors
        needs = any(t in ("xor", "sub") for t in names)
        if needs and base is None:
            raise ValueError(what + ": the object holds \"xor\" or \"sub\" tensors and needs its base")
        braw = _bases(base, obj.dtypes, obj.shapes, obj.device) if needs else None
        seg_log = getattr(obj, "segment_log", None)
        out = [None] * len(obj.dtypes)
        for g in obj.groups:
            E, sizes = g["elem_bytes"], g["sizes"]
            offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            blocks = self.planes_block_bound(sum(sizes), len(sizes), E, obj.block_size_id)
            tr = [names[i] for i in g["index"]]
            dst = None if braw is None else _base_copy(braw, g, obj.device)       # (a copy: rebuilt in place, the bases stay)
            if strides is not None and seg_log is not None:
                dst, res = tensor_decompress_seg_each_stride_dbatch(self, g["frames"], g["frame_offsets"], offs, E, seg_log, tr, [strides[i] for i in g["index"]], dst,
                                                                    g["seg_first"], dst=dst, max_total_blocks=blocks)
            elif strides is not None:
                dst, res = tensor_decompress_each_stride_dbatch(self, g["frames"], g["frame_offsets"], offs, E, tr, [strides[i] for i in g["index"]], dst, dst=dst,
                                                                max_total_blocks=blocks)
            elif seg_log is not None:
                dst, res = tensor_decompress_seg_each_dbatch(self, g["frames"], g["frame_offsets"], offs, E, seg_log, tr, dst, g["seg_first"], dst=dst,
                                                             max_total_blocks=blocks)
            else:
                dst, res = tensor_decompress_each_dbatch(self, g["frames"], g["frame_offsets"], offs, E, tr, dst, dst=dst, max_total_blocks=blocks)
            got = res.cpu().tolist()
            if got != sizes:
                raise RuntimeError("%s: element size %d, results %s for tensors of %s bytes" % (what, E, got[:8], sizes[:8]))
            for k, i in enumerate(g["index"]):
                out[i] = dst[int(offs[k]):int(offs[k + 1])].clone().view(obj.dtypes[i]).reshape(obj.shapes[i])
        return out

    setattr(FseHip, "compress_tensors_each", compress_tensors_each)

    def _window_list(what, obj, windows):
        """the `windows` of a user-facing window call -> per tensor None or (start, stop) as ints"""
        windows = list(windows)
        if len(windows) != len(obj.dtypes):
            raise ValueError("%s: %d windows for %d tensors" % (what, len(windows), len(obj.dtypes)))
        wins = []
        for k, (w, sh) in enumerate(zip(windows, obj.shapes)):
            if w is None:
                wins.append(None)
                continue
            numel = int(np.prod(sh, dtype=np.int64))
            if (not isinstance(w, (tuple, list)) or len(w) != 2 or any(not isinstance(x, numbers.Integral) or isinstance(x, bool) for x in w)
                    or not 0 <= w[0] <= w[1] <= numel):
                raise ValueError("%s: window %d is %r, (start, stop) with 0 <= start <= stop <= %d is needed" % (what, k, w, numel))
            wins.append((int(w[0]), int(w[1])))
        return wins

    def _read_windows(what, obj, wins, braw, read):
        """the groups of `obj` through read(g, src_offsets, windows, dst_offsets, dst) -> (dst, results); dst: the windows of the bases (a
        copy: rebuilt in place, the bases stay) where there are bases"""
        out = [None] * len(obj.dtypes)
        for g in obj.groups:
            E, sizes = g["elem_bytes"], g["sizes"]
            gw = [wins[i] or (0, 0) for i in g["index"]]
            if not any(b > a for a, b in gw):
                for k, i in enumerate(g["index"]):
                    if wins[i] is not None:
                        out[i] = torch.empty(0, dtype=obj.dtypes[i], device=obj.device)
                continue
            soff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            doff = np.concatenate([[0], np.cumsum([E * (b - a) for a, b in gw])]).astype(np.uint64)
            dst = None
            if braw is not None:
                dst = torch.cat([braw[i][E * a:E * b] for i, (a, b) in zip(g["index"], gw)])
            dst, res = read(g, soff, gw, doff, dst)
            got, want = res.cpu().tolist(), [E * (b - a) for a, b in gw]
            if got != want:
                raise RuntimeError("%s: element size %d, results %s for windows of %s bytes" % (what, E, got[:8], want[:8]))
            for k, i in enumerate(g["index"]):
                if wins[i] is not None:
                    out[i] = dst[int(doff[k]):int(doff[k + 1])].clone().view(obj.dtypes[i])
        return out

    def decompress_tensor_windows(self, obj, windows, base=None):
        """-> per tensor of `obj` (a CompressedTensors of compress_tensors_segmented) the elements [start, stop) of the FLATTENED tensor as a 1-D
        tensor of the recorded dtype that owns its memory: a row shard, a slice, a row range.  `windows` has one entry per tensor: None (the
        tensor is skipped and None is returned in its place) or (start, stop) with 0 <= start <= stop <= numel.  Only the segment frames that
        hold a window are decoded (tensor_decompress_window_dbatch): time and scratch follow the windows, not the tensors.
        base: for an object with `delta` set, the WHOLE base tensors as decompress_tensors takes them; the call slices them and does not change
        them.  ValueError for an object without segment_log, a window that is not one, a wrong number of windows, and a base / delta
        mismatch as in decompress_tensors -- all before any launch.  `base_digests` of the object are NOT checked here: a digest covers a whole
        base tensor and would cost more than the window saves.
        Which call takes which object: this one takes plain and delta objects of compress_tensors_segmented and refuses (ValueError) objects
        with a transform per tensor (compress_tensors_each), with predicted planes (PredictedPlanes) and with sparse planes;
        decompress_tensor_windows_each takes all of these but the sparse ones."""
        what = "decompress_tensor_windows"
        seg_log = getattr(obj, "segment_log", None)
        if seg_log is None:
            raise ValueError(what + ": the object is not segmented (compress_tensors_segmented writes those)")
        _not_sparse(obj, what)
        base, op = _read_base(obj, base, what)
        wins = _window_list(what, obj, windows)
        braw = None if base is None else _bases(base, obj.dtypes, obj.shapes, obj.device)
        return _read_windows(what, obj, wins, braw, lambda g, soff, gw, doff, dst: self.tensor_decompress_window_dbatch(
            g["frames"], g["frame_offsets"], soff, gw, doff, g["elem_bytes"], seg_log, g["seg_first"], base=dst, dst=dst, block_size_id=obj.block_size_id, delta_op=op))

    def decompress_tensor_windows_each(self, obj, windows, base=None):
        """decompress_tensor_windows for ANY segmented object that is not sparse, with the same contract -- None entries, 1-D results of the
        recorded dtype that own their memory, the whole base tensors sliced by the call and not changed, only the segment frames that hold a
        window decoded (tensor_decompress_window_each_dbatch):
          an object of compress_tensors_each(..., segment_log=...), also reopened from an archive: obj.transforms, per tensor; base where one
            of them is "xor" or "sub";
          an object written with PredictedPlanes (predictor "prev"): every tensor "pred", no base;
          a plain or a delta object of compress_tensors_segmented: every tensor "plain", or "xor" / "sub" by the object's delta_op with its base.
        A window of a "pred" tensor may start anywhere: the differences of its run in front of it lie in its first selected segment.
        ValueError before any launch: no segment_log; a sparse object; a window that is not one or a wrong number of windows; a predictor
        other than "prev"; "xor" / "sub" tensors without a base; a base for an object that holds neither.  base_digests are not checked."""
        return _read_windows_each(self, "decompress_tensor_windows_each", obj, windows, base, False)

    def decompress_tensor_windows_each_stride(self, obj, windows, base=None):
        """decompress_tensor_windows_each for objects that hold a stride above 1 as well, with the same contract and the same refusals but that
        one (tensor_decompress_window_each_stride_dbatch).  It takes everything decompress_tensor_windows_each takes -- the stride is then 1
        everywhere -- and
          an object of compress_tensors_each(..., strides=..., segment_log=...): obj.strides, one integer 1 .. 8 per tensor, validated as
            decompress_tensors validates them;
          a segmented object written with PredictedPlanes(codec, stride=S) (predictor "prev<S>"): every tensor "pred" at stride S;
          all of these reopened from an archive or a file.
        A window may start anywhere: a run is 1024 elements counted from the tensor's start at every stride, and the differences of all S
        chains in front of the window lie in its first selected segment.  ValueError before any launch: those of
        decompress_tensor_windows_each; strides that are not one integer 1 .. 8 per tensor; a predictor that predictor_stride does not know."""
        return _read_windows_each(self, "decompress_tensor_windows_each_stride", obj, windows, base, True)

    def _read_windows_each(self, what, obj, windows, base, strided):
        """the body of decompress_tensor_windows_each (strided False: an object with a stride above 1 is refused) and of
        decompress_tensor_windows_each_stride"""
        seg_log = getattr(obj, "segment_log", None)
        if seg_log is None:
            raise ValueError(what + ": the object is not segmented (compress_tensors_each and compress_tensors_segmented write those with a segment_log)")
        if getattr(obj, "sparse_permille", None) is not None:
            raise ValueError(what + ": the object holds sparse planes (SparsePlanes); windows of those are not supported")
        if not strided and any(st != 1 for st in (getattr(obj, "strides", None) or ())):
            raise ValueError(what + ": the object holds a stride above 1 (compress_tensors_each with strides); windows of those are not supported here, "
                             "decompress_tensor_windows_each_stride takes them")
        strides = _obj_strides(obj, what) if strided else None
        n = len(obj.dtypes)
        names, predictor = getattr(obj, "transforms", None), getattr(obj, "predictor", None)
        if names is not None:
            names = list(names)
            if len(names) != n or any(t not in EST_NAMES for t in names):
                raise ValueError("%s: transforms %r; one name per tensor (%d) out of %r is needed" % (what, names[:8], n, EST_NAMES))
            if predictor is not None:
                raise ValueError(what + ": a predictor does not go with a transform per tensor")
            if isinstance(base, DeltaBase):
                base = base.tensors
            if any(t in ("xor", "sub") for t in names) != (base is not None):
                raise ValueError(what + ": the object holds \"xor\" or \"sub\" tensors and needs its base" if base is None else
                                 what + ": the object holds no \"xor\" or \"sub\" tensor, a base does not belong to it")
        elif predictor is not None:
            if strided:
                strides = [predictor_stride(predictor, what)] * n
            elif predictor != "prev":
                raise ValueError("%s: predictor %r; only \"prev\" is known (decompress_tensor_windows_each_stride takes \"prev2\" .. \"prev%d\")" %
                                 (what, predictor, PRED_MAX_STRIDE))
            if base is not None:
                raise ValueError(what + ": the object holds predicted planes, a base does not belong to it")
            names = ["pred"] * n
        else:
            base, op = _read_base(obj, base, what)
            names = [("plain" if base is None else "sub" if op else "xor")] * n
        wins = _window_list(what, obj, windows)
        braw = None if base is None else _bases(base, obj.dtypes, obj.shapes, obj.device)
        if strided:
            return _read_windows(what, obj, wins, braw, lambda g, soff, gw, doff, dst: self.tensor_decompress_window_each_stride_dbatch(
                g["frames"], g["frame_offsets"], soff, gw, doff, g["elem_bytes"], seg_log, [names[i] for i in g["index"]],
                None if strides is None else [strides[i] for i in g["index"]], g["seg_first"], base=dst, dst=dst, block_size_id=obj.block_size_id))
        return _read_windows(what, obj, wins, braw, lambda g, soff, gw, doff, dst: self.tensor_decompress_window_each_dbatch(
            g["frames"], g["frame_offsets"], soff, gw, doff, g["elem_bytes"], seg_log, [names[i] for i in g["index"]], g["seg_first"], base=dst, dst=dst,
            block_size_id=obj.block_size_id))

    for f in (planes_window_first, planes_select_window_dbatch, planes_fold_window_dbatch, tensor_decompress_window_dbatch, decompress_tensor_windows,
              decompress_tensor_windows_each, decompress_tensor_windows_each_stride):
        setattr(FseHip, f.__name__, f)
    for f in (estimate_tensors, compress_tensors_auto):
        setattr(FseHip, f.__name__, f)
    for f in (planes_block_bound, planes_split_dbatch, planes_merge_dbatch, tensor_compress_dbatch, tensor_decompress_dbatch, compress_tensors, decompress_tensors,
              planes_split_xor_dbatch, planes_merge_xor_dbatch, tensor_compress_delta_dbatch, tensor_decompress_delta_dbatch, tensor_compress_mixed_dbatch,
              planes_segment_first, planes_segments_dbatch, planes_fold_segments_dbatch, tensor_compress_seg_dbatch, tensor_decompress_seg_dbatch, compress_tensors_segmented):
        setattr(FseHip, f.__name__, f)


_planes_methods()
_DEFAULT = None


def _default():
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = FseHip()
    return _DEFAULT


def compress_tensors(tensors, codec=0, block_size_id=5, base=None):
    """FseHip.compress_tensors on a library handle of the module's own"""
    return _default().compress_tensors(tensors, codec, block_size_id, base)


def compress_tensors_segmented(tensors, segment_log=18, codec=0, block_size_id=5, base=None):
    """FseHip.compress_tensors_segmented on a library handle of the module's own"""
    return _default().compress_tensors_segmented(tensors, segment_log, codec, block_size_id, base)


def decompress_tensors(obj, base=None):
    """FseHip.decompress_tensors on a library handle of the module's own"""
    return _default().decompress_tensors(obj, base)


def estimate_tensors(tensors, base=None, candidates=None, margin_permille=50):
    """FseHip.estimate_tensors on a library handle of the module's own"""
    return _default().estimate_tensors(tensors, base, candidates, margin_permille)


def compress_tensors_auto(tensors, base=None, codec=0, block_size_id=5, segment_log=None, margin_permille=50):
    """FseHip.compress_tensors_auto on a library handle of the module's own"""
    return _default().compress_tensors_auto(tensors, base, codec, block_size_id, segment_log, margin_permille)


def compress_tensors_each(tensors, transforms="auto", base=None, codec=0, block_size_id=5, segment_log=None, margin_permille=50):
    """FseHip.compress_tensors_each on a library handle of the module's own"""
    return _default().compress_tensors_each(tensors, transforms, base, codec, block_size_id, segment_log, margin_permille)


def decompress_tensor_windows(obj, windows, base=None):
    """FseHip.decompress_tensor_windows on a library handle of the module's own"""
    return _default().decompress_tensor_windows(obj, windows, base)


def decompress_tensor_windows_each(obj, windows, base=None):
    """FseHip.decompress_tensor_windows_each on a library handle of the module's own"""
    return _default().decompress_tensor_windows_each(obj, windows, base)


def decompress_tensor_windows_each_stride(obj, windows, base=None):
    """FseHip.decompress_tensor_windows_each_stride on a library handle of the module's own"""
    return _default().decompress_tensor_windows_each_stride(obj, windows, base)


def patch_tensor_windows(obj, tensors, windows, base=None):
    """FseHip.patch_tensor_windows on a library handle of the module's own"""
    return _default().patch_tensor_windows(obj, tensors, windows, base)


def patch_tensor_windows_each(obj, tensors, windows, base=None):
    """FseHip.patch_tensor_windows_each on a library handle of the module's own"""
    return _default().patch_tensor_windows_each(obj, tensors, windows, base)


def patch_tensor_windows_each_stride(obj, tensors, windows, base=None):
    """FseHip.patch_tensor_windows_each_stride on a library handle of the module's own"""
    return _default().patch_tensor_windows_each_stride(obj, tensors, windows, base)


def tensor_digests(tensors):
    """FseHip.tensor_digests on a library handle of the module's own"""
    return _default().tensor_digests(tensors)


def archive_tensors(obj):
    """FseHip.archive_tensors on a library handle of the module's own"""
    return _default().archive_tensors(obj)


def open_archive(buf):
    """FseHip.open_archive on a library handle of the module's own"""
    return _default().open_archive(buf)


def save_tensors(obj, path):
    """FseHip.save_tensors on a library handle of the module's own"""
    return _default().save_tensors(obj, path)


def load_tensors(path, device="cuda"):
    """FseHip.load_tensors on a library handle of the module's own"""
    return _default().load_tensors(path, device)


# ---------------------------------------------------------------------------------------------------------
#  FSE for 16-bit symbols (lib/fseU16.h): sizes of the uncompressed side are in symbols
# ---------------------------------------------------------------------------------------------------------
FSEU16_MAX_SYMBOL_VALUE = 286


def fse_u16_compress_bound(n_symbols):      # FSE_compressBound over the bytes of the symbols (what programs/bench.c:221 hands over)
    return fse_compress_bound(2 * n_symbols)


def _u16_methods():
    def _blocks16(t, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int16 or t.dim() != 2:
            raise TypeError("%s must be a 2-D CUDA int16 tensor (16-bit symbols; torch has no uint16 arithmetic, the bits are what counts)" % what)
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError("%s: symbols of a block must be contiguous" % what)
        return t

    def fse_count_u16_batch(self, src, sizes=None, max_symbol_value=FSEU16_MAX_SYMBOL_VALUE):
        n = _blocks16(src, "src").shape[0]
        counts = torch.empty((n, FSEU16_MAX_SYMBOL_VALUE + 1), dtype=torch.int32, device=src.device)
        maxsv = torch.empty(n, dtype=torch.int32, device=src.device)
        results = torch.empty(n, dtype=torch.int64, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_FSE_countU16_batch(_ptr(counts), _ptr(maxsv), _ptr(results), _ptr(src), SZ(2 * src.stride(0)), ps, uni,
                                                  C.c_uint(max_symbol_value), SZ(n), _stream()), "FSE_countU16_batch")
        return counts, maxsv, results

    def fse_compress_u16_batch(self, src, table_log=0, max_symbol_value=0, sizes=None, dst=None, dst_capacity=None, results=None, workspace=None):
        n = _blocks16(src, "src").shape[0]
        cap = fse_u16_compress_bound(src.shape[1]) if dst_capacity is None else dst_capacity
        g = None
        if dst is None:
            dst, g = self._dst(n, cap, src.device)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=src.device)
        if workspace is None:
            workspace = torch.empty(int(self.lib.FSEHIP_FSE_compressU16_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=src.device)
        ps, uni, keep = _sizes_arg(src.shape[1] if sizes is None else sizes, src)
        _check(self.lib.FSEHIP_FSE_compressU16_batch(_ptr(dst), SZ(dst.stride(0)), SZ(cap), _ptr(results), _ptr(src), SZ(2 * src.stride(0)), ps, uni,
                                                     C.c_uint(max_symbol_value), C.c_uint(table_log), SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()),
               "FSE_compressU16_batch")
        if g:
            g.check("FSE_compressU16_batch")
        return dst, results

    def fse_decompress_u16_batch(self, csrc, csizes, dst_capacity, dst=None, results=None, workspace=None):
        n = _blocks(csrc, "csrc").shape[0]
        g = None
        if dst is None:
            dst, g = self._dst(n, dst_capacity, csrc.device, dtype=torch.int16)
        if results is None:
            results = torch.empty(n, dtype=torch.int64, device=csrc.device)
        if workspace is None:
            workspace = torch.empty(int(self.lib.FSEHIP_FSE_decompressU16_batch_workspaceSize(SZ(n))), dtype=torch.uint8, device=csrc.device)
        ps, uni, keep = _sizes_arg(csizes, csrc)
        _check(self.lib.FSEHIP_FSE_decompressU16_batch(_ptr(dst), SZ(2 * dst.stride(0)), SZ(dst_capacity), _ptr(results), _ptr(csrc), SZ(csrc.stride(0)), ps, uni,
                                                       SZ(n), _ptr(workspace), SZ(workspace.numel()), _stream()), "FSE_decompressU16_batch")
        if g:
            g.check("FSE_decompressU16_batch")
        return dst, results

    # host pointers, reference signatures
    def fse_count_u16(self, src, max_sv=FSEU16_MAX_SYMBOL_VALUE):
        src = np.ascontiguousarray(src, dtype=np.uint16)
        count = np.zeros(max(max_sv, FSEU16_MAX_SYMBOL_VALUE) + 1, dtype=np.uint32)
        msv = C.c_uint(max_sv)
        r = int(self.lib.FSEHIP_FSE_countU16(count.ctypes.data_as(VP), C.byref(msv), src.ctypes.data_as(VP), SZ(src.size)))
        return r, count, int(msv.value)

    def fse_compress_u16(self, src, max_sv=0, table_log=0, cap=None):
        src = np.ascontiguousarray(src, dtype=np.uint16)
        cap = fse_u16_compress_bound(src.size) if cap is None else cap
        out = np.zeros(max(cap, 1) + 16, dtype=np.uint8)
        out[cap:] = 0xA5
        r = int(self.lib.FSEHIP_FSE_compressU16(out.ctypes.data_as(VP), SZ(cap), src.ctypes.data_as(VP), SZ(src.size), C.c_uint(max_sv), C.c_uint(table_log)))
        assert (out[cap:] == 0xA5).all(), "FSE_compressU16 wrote past dstCapacity"
        return r, out[:cap]

    def fse_decompress_u16(self, csrc, cap):
        csrc = np.ascontiguousarray(csrc, dtype=np.uint8)
        out = np.zeros(max(cap, 1) + 8, dtype=np.uint16)
        out[cap:] = 0xA5A5
        r = int(self.lib.FSEHIP_FSE_decompressU16(out.ctypes.data_as(VP), SZ(cap), csrc.ctypes.data_as(VP), SZ(csrc.size)))
        assert (out[cap:] == 0xA5A5).all(), "FSE_decompressU16 wrote past dstCapacity"
        return r, out[:cap]

    for f in (fse_count_u16_batch, fse_compress_u16_batch, fse_decompress_u16_batch, fse_count_u16, fse_compress_u16, fse_decompress_u16):
        setattr(FseHip, f.__name__, f)


_u16_methods()
