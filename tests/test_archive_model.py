"""Tensor archives without a device (include/fsehip.h, "tensor archives"): the numpy model of archive_corpus.py -- build and parse are each
other's inverse over every flag combination, count and meta size; headBytes at the three residues where its rounding can go wrong -- then the
library's host arithmetic against it (FSEHIP_archive_headBytes, FSEHIP_archive_inspect: one refusal per header rule), every argument refusal
of the two device calls decided before any device call with nothing written, and the Python surface with the pinned signatures."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest

import archive_corpus as ac
from archive_corpus import CODECS, CORRUPT, DELTA, DIGESTS, GENERIC, SPARSE, SRC_WRONG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint
EXPORTS = ("FSEHIP_archive_headBytes", "FSEHIP_archive_inspect", "FSEHIP_archive_workspaceBound", "FSEHIP_archive_seal_dbatch", "FSEHIP_archive_open_dbatch")
ALL_FLAGS = range(16)


class Info(C.Structure):
    _fields_ = [("magic", C.c_char * 4), ("version", C.c_uint16), ("flags", C.c_uint16), ("elem_bytes", C.c_uint8), ("block_size_id", C.c_uint8),
                ("seg_log", C.c_uint8), ("delta_op", C.c_uint8), ("sparse_permille", C.c_uint16), ("reserved", C.c_uint16), ("n_tensors", C.c_uint64),
                ("n_frames", C.c_uint64), ("total_bytes", C.c_uint64), ("max_total_blocks", C.c_uint64), ("meta_bytes", C.c_uint64), ("frames_bytes", C.c_uint64),
                ("head_bytes", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    lib = C.CDLL(path)
    for name in EXPORTS[:3]:
        getattr(lib, name).restype = SZ
    return lib


def _signed(r):
    return r - (1 << 64) if r >= 1 << 63 else r


def _example(flags, nT, meta_bytes, seed=0, E=2, seg_log=0):
    """a consistent archive head's ingredients: (fields, sizes, offsets, digests, codecs, meta)"""
    rng = np.random.default_rng(1000 * flags + 10 * nT + meta_bytes + seed)
    sizes = [int(x) for x in rng.integers(0, 5000, nT)]
    nF = ac.seg_first(sizes, E, seg_log)[-1] if seg_log else nT * E
    offsets = [int(x) for x in np.concatenate([[0], np.cumsum(rng.integers(11, 300, nF))])]
    f = ac.fields(E, nT, nF, sum(sizes), offsets[-1], flags, block_size_id=0, seg_log=seg_log, delta_op=1 if flags & DELTA else 0,
                  sparse_permille=500 if flags & SPARSE else 0, max_total_blocks=nF + 7, meta_bytes=meta_bytes)
    digests = [int(x) for x in rng.integers(0, 1 << 63, nT)] if flags & DIGESTS else None
    codecs = bytes(rng.integers(0, 2, nF, dtype=np.uint8)) if flags & CODECS else None
    return f, sizes, offsets, digests, codecs, bytes(rng.integers(1, 256, meta_bytes, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------- 1: the model
def test_magic_is_no_frame_magic(restatement):
    data = np.arange(300, dtype=np.uint8)
    for codec in (0, 1):
        r, frame = restatement.frame_compress(data, 0, codec)
        assert r > 4 and bytes(frame[:4]) != ac.MAGIC
    assert ac.MAGIC == b"FSTA" and ac.HEADER.size == 64


def test_build_and_parse_are_inverses():
    for flags, nT, mb in itertools.product(ALL_FLAGS, (0, 1, 3, 1025), (0, 1, 7, 8, 9)):
        y = _example(flags, nT, mb)
        x = ac.build(*y)
        assert len(x) % 256 == 0 and len(x) == ac.head_bytes(nT, y[0]["n_frames"], flags, mb), (flags, nT, mb)
        back = ac.parse(x)
        assert back == y, (flags, nT, mb)
        assert (ac.build(*back) == x).all(), (flags, nT, mb)
    seg = _example(DELTA | CODECS, 3, 5, E=1, seg_log=10)
    assert seg[0]["n_frames"] > 3 and ac.parse(ac.build(*seg)) == seg


def test_head_bytes_at_the_residues_of_its_rounding():
    # E = 1, no flags: the unpadded head is 64 + 8 nT + 8 (nT + 1) + (meta rounded to 8) + 8
    for nT, mb, residue, head in ((11, 0, 0, 256), (11, 1, 8, 512), (10, 1, 248, 256), (27, 0, 0, 512), (26, 8, 248, 512)):
        assert ac.unpadded(nT, nT, 0, mb) % 256 == residue and ac.head_bytes(nT, nT, 0, mb) == head, (nT, mb)
    r = ac.regions(3, 6, CODECS | DIGESTS | DELTA, 9)
    assert [r[k] for k in ("sizes", "offsets", "digests", "codecs", "meta", "pad", "digest")] == [64, 88, 144, 168, 176, 192, 248]


def test_seal_and_open_models():
    f, sizes, offsets, digests, codecs, meta = _example(CODECS | DIGESTS | DELTA, 3, 9)
    S = [0] + [int(x) for x in np.cumsum(sizes)]
    results = [b - a for a, b in zip(offsets, offsets[1:])]
    head, res = ac.seal(dict(f, frames_bytes=0), S, offsets, results, sizes, 1 << 20, digests, codecs, meta)
    assert res == len(head) + offsets[-1] and (head == ac.build(f, sizes, offsets, digests, codecs, meta)).all()
    opened = ac.open_(head, f)
    assert opened["verdict"] == res and opened["src_offsets"] == S and opened["frame_offsets"] == offsets and opened["digests"] == digests
    assert bytes(opened["codecs"]) == codecs and opened["seg_first"] is None
    for kw, want in ((dict(frame_results=[-1] + results[1:]), GENERIC), (dict(capacity=len(head) + offsets[-1] - 1), ac.TOO_SMALL),
                     (dict(tensor_results=[sizes[0], -1, sizes[2]]), GENERIC), (dict(codecs=b"\x02" + codecs[1:]), GENERIC)):
        args = dict(src_offsets=S, frame_offsets=offsets, frame_results=results, tensor_results=sizes, capacity=1 << 20, digests=digests, codecs=codecs, meta=meta)
        args.update(kw)
        bad, r = ac.seal(f, **args)
        assert r == want and not bad[:4].any() and ac.header_error(ac.header_fields(bad), 1 << 20) == GENERIC, kw
    damaged = head.copy()
    damaged[70] ^= 1
    for h in (damaged, ac.restamp(damaged.copy())):
        got = ac.open_(h, f)
        assert got["verdict"] == CORRUPT and got["frame_offsets"] == [0] * len(offsets)


# ---------------------------------------------------------------------------------------------------------------- 2: the host arithmetic
def _inspect(lib, f, archive_bytes):
    info = Info()
    raw = ac.header(f)
    r = _signed(lib.FSEHIP_archive_inspect(C.byref(info), raw, U64(archive_bytes)))
    return r, info


def test_head_bytes_and_inspect_against_the_model(lib):
    for flags, nT, mb in itertools.product(ALL_FLAGS, (0, 1, 3, 1025), (0, 1, 7, 8, 9)):
        for E, seg_log in ((2, 0), (8, 0), (4, 11)):
            f = _example(flags, nT, mb, E=E, seg_log=seg_log)[0]
            want = ac.head_bytes(nT, f["n_frames"], flags, mb)
            assert lib.FSEHIP_archive_headBytes(U64(nT), U64(f["n_frames"]), UI(flags), U64(mb)) == want
            size = want + f["frames_bytes"]
            r, info = _inspect(lib, f, size)
            assert r == ac.header_error(f, size) == (CORRUPT if flags & DIGESTS and not flags & DELTA else want), (flags, nT, mb, E)
            if r > 0:
                assert info.head_bytes == want and {k: getattr(info, k) for k in ac.FIELDS} == f
    for nT, mb in ((11, 0), (11, 1), (10, 1)):
        assert lib.FSEHIP_archive_headBytes(U64(nT), U64(nT), UI(0), U64(mb)) == ac.head_bytes(nT, nT, 0, mb)
    for nT, nF, flags, mb in ((1 << 24, 0, 0, 0), (0, 1 << 31, 0, 0), (0, 0, 16, 0), (0, 0, 0, 1 << 31), (1 << 61, 0, 0, 0), (0, 1 << 61, 0, 0), (0, 0, 0, (1 << 64) - 1)):
        assert _signed(lib.FSEHIP_archive_headBytes(U64(nT), U64(nF), UI(flags), U64(mb))) == GENERIC == ac.head_bytes(nT, nF, flags, mb)
    bound = lib.FSEHIP_archive_workspaceBound
    b0, b1 = bound(U64(0), U64(0), U64(256)), bound(U64(1025), U64(4100), U64(ac.head_bytes(1025, 4100, 0, 0)))
    assert 0 < b0 <= b1 < (1 << 24) and b0 % 256 == b1 % 256 == 0
    for nT, nF, head in ((1 << 24, 0, 256), (0, 1 << 31, 256), (0, 0, 0), (0, 0, 264), (0, 0, 1 << 40)):
        assert _signed(bound(U64(nT), U64(nF), U64(head))) == GENERIC


GOOD = dict(elem_bytes=2, n_tensors=3, n_frames=6, total_bytes=1000, frames_bytes=700, flags=DELTA | SPARSE, delta_op=1, sparse_permille=500, max_total_blocks=9,
            meta_bytes=5)
# one refusal per header rule: the field at its first illegal value, the couplings, the overflows
REFUSALS = [
    ("magic", dict(magic=b"FSTB"), GENERIC), ("magic of a sealed-and-refused head", dict(magic=b"\0\0\0\0"), GENERIC),
    ("version 0", dict(version=0), GENERIC), ("version 2", dict(version=2), GENERIC),
    ("an unknown flag bit", dict(flags=16 | DELTA | SPARSE), CORRUPT), ("the top flag bit", dict(flags=0x8000 | DELTA | SPARSE), CORRUPT),
    ("DIGESTS without DELTA", dict(flags=DIGESTS, delta_op=0, sparse_permille=0), CORRUPT),
    ("elemBytes 0", dict(elem_bytes=0), CORRUPT), ("elemBytes 3", dict(elem_bytes=3, n_frames=9), CORRUPT), ("elemBytes 16", dict(elem_bytes=16, n_frames=48), CORRUPT),
    ("blockSizeId 7", dict(block_size_id=7), CORRUPT),
    ("segLog 9", dict(seg_log=9), CORRUPT), ("segLog 10 at blockSizeId 1", dict(seg_log=10, block_size_id=1), CORRUPT), ("segLog 31", dict(seg_log=31), CORRUPT),
    ("deltaOp 2", dict(delta_op=2), CORRUPT), ("deltaOp without DELTA", dict(flags=SPARSE), CORRUPT),
    ("sparsePermille 1001", dict(sparse_permille=1001), CORRUPT), ("sparsePermille without SPARSE", dict(flags=DELTA), CORRUPT),
    ("the reserved field", dict(reserved=1), CORRUPT),
    ("nTensors 2^24", dict(n_tensors=1 << 24, n_frames=1 << 25), CORRUPT), ("nFrames 2^31", dict(n_frames=1 << 31, seg_log=10), CORRUPT),
    ("metaBytes 2^31", dict(meta_bytes=1 << 31), CORRUPT), ("maxTotalBlocks 2^31", dict(max_total_blocks=1 << 31), CORRUPT),
    ("totalBytes 2^46", dict(total_bytes=1 << 46), CORRUPT), ("a launch of 2^24 workgroups", dict(total_bytes=((1 << 24) - 4) << 15), CORRUPT),
    ("nFrames above nTensors * E, unsegmented", dict(n_frames=7), CORRUPT), ("nFrames below nTensors * E, unsegmented", dict(n_frames=5), CORRUPT),
    ("nFrames below nTensors * E, segmented", dict(n_frames=5, seg_log=10), CORRUPT),
    ("bytes in no tensors", dict(n_tensors=0, n_frames=0, total_bytes=1), CORRUPT),
    ("8 * nTensors overflows", dict(n_tensors=1 << 61, n_frames=1 << 62), CORRUPT), ("8 * nFrames overflows", dict(n_frames=1 << 61, seg_log=10), CORRUPT),
    ("headBytes + framesBytes overflows", dict(frames_bytes=(1 << 64) - 1), SRC_WRONG), ("headBytes + framesBytes overflows by one", dict(frames_bytes=(1 << 64) - 256), SRC_WRONG),
]


def test_inspect_refuses_every_header_rule(lib):
    good = ac.fields(**GOOD)
    head = ac.head_bytes(3, 6, good["flags"], 5)
    size = head + 700
    assert head == 256 and _inspect(lib, good, size)[0] == ac.header_error(good, size) == head
    assert _inspect(lib, dict(good, seg_log=10, n_frames=8), size)[0] == head, "segmented: more frames than planes"
    assert _inspect(lib, dict(good, total_bytes=((1 << 24) - 5) << 15), size)[0] == head, "the largest launch"
    for name, change, want in REFUSALS:
        f = dict(good, **change)
        r, info = _inspect(lib, f, 1 << 62)
        assert r == want == ac.header_error(f, 1 << 62), name
        assert info.head_bytes == 0, name
    # the archive's size: one byte short of the header, of the head, of head and frames
    for nbytes, want in ((63, SRC_WRONG), (64, SRC_WRONG), (head - 1, SRC_WRONG), (head, SRC_WRONG), (size - 1, SRC_WRONG), (size, head), (size + 1, head)):
        assert _inspect(lib, good, nbytes)[0] == want == ac.header_error(good, nbytes), nbytes
    assert _inspect(lib, dict(good, frames_bytes=0), head)[0] == head
    info = Info()
    assert _signed(lib.FSEHIP_archive_inspect(None, ac.header(good), U64(size))) == GENERIC and _signed(lib.FSEHIP_archive_inspect(C.byref(info), None, U64(size))) == GENERIC


# ---------------------------------------------------------------------------------------------------------------- 3: the device calls' arguments
def _info(f, head=None):
    info = Info(*[f[k] for k in ac.FIELDS])
    info.head_bytes = ac.head_bytes(f["n_tensors"], f["n_frames"], f["flags"], f["meta_bytes"]) if head is None else head
    return info


def test_bad_arguments_of_the_device_calls_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 64)()
    room = (C.c_uint8 * 4096)()
    p, null = C.cast(a, VP), VP(0)
    assert p.value % 8 == 0
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)
    full = ac.fields(2, 3, 8, 1000, 700, CODECS | DIGESTS | DELTA, seg_log=10, delta_op=1, meta_bytes=5)
    plain = ac.fields(2, 3, 6, 1000, 700)
    head = ac.head_bytes(3, 8, full["flags"], 5)
    need = lib.FSEHIP_archive_workspaceBound(U64(3), U64(8), U64(head))

    def seal(f=full, ptrs=None, info="ok", cap=1 << 20, w=ws, wb=big):      # ptrs: archive, result, S, F, FR, TR, codecs, digests, meta
        q = list(ptrs or [p] * 9)
        i = C.byref(_info(f)) if info == "ok" else info
        return lib.FSEHIP_archive_seal_dbatch(q[0], U64(cap), q[1], i, q[2], q[3], q[4], q[5], q[6], q[7], q[8], w, wb, null)

    def open_(f=full, ptrs=None, info="ok", nbytes=1 << 20, w=ws, wb=big):  # ptrs: S, F, codecs, digests, segFirst, verdict, archive
        q = list(ptrs or [p] * 7)
        i = C.byref(_info(f)) if info == "ok" else info
        return lib.FSEHIP_archive_open_dbatch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], U64(nbytes), i, w, wb, null)

    for k in range(9):                                                      # every array: null (all nine are needed under `full`)
        q = [p] * 9
        q[k] = null
        assert seal(ptrs=q) == HIP_INVALID_VALUE, k
    for k in range(7):
        q = [p] * 7
        q[k] = null
        assert open_(ptrs=q) == HIP_INVALID_VALUE, k
    odd = VP(p.value + 4)
    assert seal(ptrs=[odd] + [p] * 8) == HIP_INVALID_VALUE and open_(ptrs=[p] * 6 + [odd]) == HIP_INVALID_VALUE, "d_archive off its 8-byte alignment"
    for call in (seal, open_):
        assert call(info=null) == HIP_INVALID_VALUE
        assert call(w=null) == HIP_INVALID_VALUE and call(w=null, wb=SZ(0)) == HIP_INVALID_VALUE and call(w=VP(ws.value + 8)) == HIP_INVALID_VALUE
        assert call(wb=SZ(need - 1)) == HIP_INVALID_VALUE
        assert call(info=C.byref(_info(full, head + 256))) == HIP_INVALID_VALUE and call(info=C.byref(_info(full, 0))) == HIP_INVALID_VALUE, "headBytes not that of the counts"
        for name, change, _ in REFUSALS[4:-2]:                              # an info that inspect refuses (the seal ignores magic, version and framesBytes)
            assert call(f=dict(ac.fields(**GOOD), **change)) == HIP_INVALID_VALUE, name
        assert call(f=plain, ptrs=[p] * 9 if call is seal else [p] * 7, **({"cap": 255} if call is seal else {"nbytes": 255})) == HIP_INVALID_VALUE, "shorter than the head"
    assert seal(cap=head - 1) == HIP_INVALID_VALUE
    assert open_(nbytes=head - 1) == HIP_INVALID_VALUE and open_(nbytes=head + 699) == HIP_INVALID_VALUE
    for name, change, _ in REFUSALS[:4] + REFUSALS[-2:]:
        assert open_(f=dict(full, **change)) == HIP_INVALID_VALUE, name
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- 4: Python
def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    names = ("archive_tensors", "open_archive", "save_tensors", "load_tensors")
    assert set(names) <= set(finitestateentropy_amd.__all__) and all(getattr(finitestateentropy_amd, n) is getattr(api, n) for n in names)
    assert list(inspect.signature(api.archive_tensors).parameters) == ["obj"] and list(inspect.signature(api.open_archive).parameters) == ["buf"]
    assert list(inspect.signature(api.save_tensors).parameters) == ["obj", "path"] and list(inspect.signature(api.load_tensors).parameters) == ["path", "device"]
    for name in names + ("archive_head_bytes", "archive_info", "archive_inspect", "archive_workspace_bound", "archive_seal_dbatch", "archive_open_dbatch"):
        assert callable(getattr(api.FseHip, name)), name
    assert "copied" in api.FseHip.archive_tensors.__doc__.lower() and "views" in api.FseHip.open_archive.__doc__.lower()
    assert (api.ARCHIVE_MAGIC.to_bytes(4, "little"), api.ARCHIVE_VERSION) == (ac.MAGIC, ac.VERSION)
    assert (api.ARCHIVE_CODECS, api.ARCHIVE_DIGESTS, api.ARCHIVE_SPARSE, api.ARCHIVE_DELTA) == (CODECS, DIGESTS, SPARSE, DELTA)
    assert C.sizeof(api.ArchiveInfo) == C.sizeof(Info) == 72 and [n for n, _ in api.ArchiveInfo._fields_][-1] == "headBytes"
    # the host arithmetic through the binding (no launch: nothing here has a device)
    hip = api.FseHip.__new__(api.FseHip)
    hip.lib = api._lib.load()
    assert hip.archive_head_bytes(11, 11) == 256 and hip.archive_head_bytes(11, 11, 0, 1) == 512
    info = hip.archive_info(2, 3, 6, 1000, flags=DELTA | SPARSE, block_size_id=0, delta_op="sub", sparse_permille=500, max_total_blocks=9, meta_bytes=5)
    good = ac.fields(**dict(GOOD, frames_bytes=0))
    assert bytes(info)[:64] == ac.header(good) and info.headBytes == 256
    back = hip.archive_inspect(ac.header(dict(good, frames_bytes=700)), 956)
    assert (back.framesBytes, back.headBytes, back.deltaOp, back.sparsePermille) == (700, 256, 1, 500)
    with pytest.raises(ValueError, match="corruption_detected.*segLog=9"):
        hip.archive_inspect(ac.header(dict(good, seg_log=9)), 956)
    with pytest.raises(ValueError, match="srcSize_wrong"):
        hip.archive_inspect(ac.header(dict(good, frames_bytes=700)), 955)
    with pytest.raises(ValueError):
        hip.archive_head_bytes(1 << 24, 0)
    assert hip.archive_workspace_bound(3, 6, 256) % 256 == 0
    with pytest.raises(TypeError):
        hip.archive_tensors([1, 2])
    # the pinned signatures of the three plane model tests still hold
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.compress_tensors_segmented).parameters) == ["tensors", "segment_log", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"]
    assert list(inspect.signature(api.tensor_digests).parameters) == ["tensors"]
    assert list(inspect.signature(api.DeltaBase.__init__).parameters) == ["self", "tensors", "op", "check"]
    assert list(inspect.signature(api.SparsePlanes.__init__).parameters) == ["self", "codec", "permille"]
    assert list(inspect.signature(api.CompressedTensors.__init__).parameters) == ["self", "groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"]
