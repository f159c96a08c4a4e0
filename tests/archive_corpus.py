"""The numpy model of the tensor archive (include/fsehip.h, "tensor archives"): the head of `head | frames` built from and parsed into plain
values, the header rules of FSEHIP_archive_inspect as a function of integers, the seal's and the open's verdicts, and the arrays an open
emits.  The digest is tensor_digest of planes_digest_corpus.py.  Nothing here calls the library."""
import struct

import numpy as np

import planes_digest_corpus as dg

MAGIC = b"FSTA"
VERSION = 1
CODECS, DIGESTS, SPARSE, DELTA = 1, 2, 4, 8
KNOWN = CODECS | DIGESTS | SPARSE | DELTA
HEADER = struct.Struct("<4sHHBBBBHHQQQQQQ")
FIELDS = ("magic", "version", "flags", "elem_bytes", "block_size_id", "seg_log", "delta_op", "sparse_permille", "reserved", "n_tensors", "n_frames", "total_bytes",
          "max_total_blocks", "meta_bytes", "frames_bytes")
GENERIC, TOO_SMALL, SRC_WRONG, CORRUPT = -1, -2, -3, -4
T = 32768


def _r8(n):
    return (n + 7) // 8 * 8


def regions(n_tensors, n_frames, flags, meta_bytes):
    """byte positions in the head: sizes, offsets, digests, codecs, meta, padding, the digest; the last is headBytes - 8"""
    sizes = 64
    offsets = sizes + 8 * n_tensors
    digests = offsets + 8 * (n_frames + 1)
    codecs = digests + (8 * n_tensors if flags & DIGESTS else 0)
    meta = codecs + (_r8(n_frames) if flags & CODECS else 0)
    pad = meta + _r8(meta_bytes)
    head = (pad + 8 + 255) // 256 * 256
    return dict(sizes=sizes, offsets=offsets, digests=digests, codecs=codecs, meta=meta, pad=pad, digest=head - 8)


def unpadded(n_tensors, n_frames, flags, meta_bytes):
    return regions(n_tensors, n_frames, flags, meta_bytes)["pad"] + 8


def head_bytes(n_tensors, n_frames, flags, meta_bytes):
    """FSEHIP_archive_headBytes"""
    if flags & ~KNOWN or n_tensors >= 1 << 24 or n_frames >= 1 << 31 or meta_bytes >= 1 << 31:
        return GENERIC
    return regions(n_tensors, n_frames, flags, meta_bytes)["digest"] + 8


def fields(elem_bytes=2, n_tensors=0, n_frames=None, total_bytes=0, frames_bytes=0, flags=0, block_size_id=0, seg_log=0, delta_op=0, sparse_permille=0,
           max_total_blocks=0, meta_bytes=0):
    return dict(magic=MAGIC, version=VERSION, flags=flags, elem_bytes=elem_bytes, block_size_id=block_size_id, seg_log=seg_log, delta_op=delta_op,
                sparse_permille=sparse_permille, reserved=0, n_tensors=n_tensors, n_frames=n_tensors * elem_bytes if n_frames is None else n_frames,
                total_bytes=total_bytes, max_total_blocks=max_total_blocks, meta_bytes=meta_bytes, frames_bytes=frames_bytes)


def header(f):
    return HEADER.pack(*[f[k] for k in FIELDS])


def header_fields(raw):
    return dict(zip(FIELDS, HEADER.unpack(bytes(raw[:64]))))


def header_error(f, archive_bytes):
    """FSEHIP_archive_inspect on the fields -> headBytes, or the error, rule by rule in the library's order"""
    if archive_bytes < 64:
        return SRC_WRONG
    if f["magic"] != MAGIC or f["version"] != VERSION:
        return GENERIC
    fl = f["flags"]
    if fl & ~KNOWN or (fl & DIGESTS and not fl & DELTA):
        return CORRUPT
    if f["elem_bytes"] not in (1, 2, 4, 8) or f["block_size_id"] > 6 or (f["seg_log"] and not 10 + f["block_size_id"] <= f["seg_log"] <= 30):
        return CORRUPT
    if f["delta_op"] > 1 or (f["delta_op"] and not fl & DELTA):
        return CORRUPT
    if f["sparse_permille"] > 1000 or (f["sparse_permille"] and not fl & SPARSE) or f["reserved"]:
        return CORRUPT
    if f["n_tensors"] >= 1 << 24 or f["n_frames"] >= 1 << 31 or f["meta_bytes"] >= 1 << 31 or f["max_total_blocks"] >= 1 << 31:
        return CORRUPT
    if f["total_bytes"] >= 1 << 46 or (f["total_bytes"] >> 15) + 1 + f["n_tensors"] >= 1 << 24:
        return CORRUPT
    planes = f["n_tensors"] * f["elem_bytes"]
    if (f["n_frames"] < planes) if f["seg_log"] else (f["n_frames"] != planes):
        return CORRUPT
    if f["n_tensors"] == 0 and f["total_bytes"]:
        return CORRUPT
    head = head_bytes(f["n_tensors"], f["n_frames"], fl, f["meta_bytes"])
    if head > archive_bytes or f["frames_bytes"] > archive_bytes - head:
        return SRC_WRONG
    return head


def digest_of(head):
    head = np.asarray(head, np.uint8)
    return dg.tensor_digest(head[:len(head) - 8])


def restamp(head):
    """the head with its last eight bytes recomputed (in place) -> head"""
    head[len(head) - 8:] = np.array([digest_of(head)], "<u8").view(np.uint8)
    return head


def build(f, sizes, offsets, digests=None, codecs=None, meta=b""):
    """the head as a uint8 array: f the fields, sizes / offsets / digests sequences of ints, codecs and meta bytes"""
    nT, nF, fl = f["n_tensors"], f["n_frames"], f["flags"]
    assert len(sizes) == nT and len(offsets) == nF + 1 and len(meta) == f["meta_bytes"]
    assert (digests is not None) == bool(fl & DIGESTS) and (codecs is not None) == bool(fl & CODECS)
    r = regions(nT, nF, fl, len(meta))
    head = np.zeros(r["digest"] + 8, np.uint8)
    head[:64] = np.frombuffer(header(f), np.uint8)
    head[r["sizes"]:r["offsets"]] = np.asarray(sizes, "<u8").view(np.uint8)
    head[r["offsets"]:r["digests"]] = np.asarray(offsets, "<u8").view(np.uint8)
    if digests is not None:
        assert len(digests) == nT
        head[r["digests"]:r["codecs"]] = np.asarray(digests, "<u8").view(np.uint8)
    if codecs is not None:
        assert len(codecs) == nF
        head[r["codecs"]:r["codecs"] + nF] = np.frombuffer(bytes(codecs), np.uint8)
    head[r["meta"]:r["meta"] + len(meta)] = np.frombuffer(bytes(meta), np.uint8)
    return restamp(head)


def parse(head):
    """-> (fields, sizes, offsets, digests or None, codecs or None, meta): the layout alone, no rule is checked (AssertionError where the
    padding is not zero or the digest is not the head's)"""
    head = np.asarray(head, np.uint8)
    f = header_fields(head)
    nT, nF, fl = f["n_tensors"], f["n_frames"], f["flags"]
    r = regions(nT, nF, fl, f["meta_bytes"])
    assert len(head) == r["digest"] + 8

    def u64s(a, b):
        return [int(x) for x in head[a:b].view("<u8")]
    sizes, offsets = u64s(r["sizes"], r["offsets"]), u64s(r["offsets"], r["digests"])
    digests = u64s(r["digests"], r["codecs"]) if fl & DIGESTS else None
    codecs = bytes(head[r["codecs"]:r["codecs"] + nF]) if fl & CODECS else None
    meta = bytes(head[r["meta"]:r["meta"] + f["meta_bytes"]])
    assert not head[r["codecs"] + (nF if fl & CODECS else 0):r["meta"]].any() and not head[r["meta"] + f["meta_bytes"]:r["digest"]].any()
    assert u64s(r["digest"], r["digest"] + 8) == [digest_of(head)]
    return f, sizes, offsets, digests, codecs, meta


def seg_first(sizes, E, seg_log):
    """FSEHIP_planes_segmentFirst"""
    out = [0]
    for n in sizes:
        for p in range(E):
            size = (n - p + E - 1) // E if n > p else 0
            out.append(out[-1] + max((size + (1 << seg_log) - 1) >> seg_log, 1))
    return out


def seal(f, src_offsets, frame_offsets, frame_results, tensor_results, capacity, digests=None, codecs=None, meta=b""):
    """FSEHIP_archive_seal_dbatch -> (head, result): the head as the device leaves it, with framesBytes from frame_offsets and the magic 0 on
    refusal"""
    nT, nF = f["n_tensors"], f["n_frames"]
    S, F = [int(x) for x in src_offsets], [int(x) for x in frame_offsets]
    g = dict(f, frames_bytes=F[nF])
    head_n = head_bytes(nT, nF, f["flags"], len(meta))
    bad = any(r < 0 for r in tensor_results) or any(a > b for a, b in zip(S, S[1:])) or (nT and S[nT] - S[0] != f["total_bytes"])
    bad = bad or F[0] != 0 or any(r < 0 or a > b or r > b - a for a, b, r in zip(F, F[1:], frame_results))
    bad = bad or (codecs is not None and any(c > 1 for c in bytes(codecs)))
    short = F[nF] > capacity - head_n
    head = build(g, [max(b - a, 0) for a, b in zip(S, S[1:])], F, digests, codecs, meta)
    if bad or short:
        head[:4] = 0
        return head, GENERIC if bad else TOO_SMALL
    return head, head_n + F[nF]


def open_(head, info):
    """FSEHIP_archive_open_dbatch of a head (its length is info's headBytes) -> dict(verdict, src_offsets, frame_offsets, digests, codecs,
    seg_first)"""
    head = np.asarray(head, np.uint8)
    nT, nF, fl, E = info["n_tensors"], info["n_frames"], info["flags"], info["elem_bytes"]
    r = regions(nT, nF, fl, info["meta_bytes"])
    assert len(head) == r["digest"] + 8

    def u64s(a, b):
        return [int(x) for x in head[a:b].view("<u8")]
    bad = bytes(head[:64]) != header(info)
    sizes = u64s(r["sizes"], r["offsets"])
    bad = bad or any(n > info["total_bytes"] for n in sizes)
    sizes = [n if n <= info["total_bytes"] else 0 for n in sizes]
    F = u64s(r["offsets"], r["digests"])
    bad = bad or F[0] != 0 or any(a > b for a, b in zip(F, F[1:])) or F[nF] != info["frames_bytes"]
    cod = head[r["codecs"]:r["meta"]]
    if fl & CODECS:
        bad = bad or (cod[:nF] > 1).any() or cod[nF:].any()
    bad = bad or head[r["meta"] + info["meta_bytes"]:r["digest"]].any()
    bad = bad or u64s(r["digest"], r["digest"] + 8) != [digest_of(head)]
    S = [0]
    for n in sizes:
        S.append(S[-1] + n)
    bad = bad or S[nT] != info["total_bytes"]
    first = seg_first(sizes, E, info["seg_log"]) if info["seg_log"] else None
    bad = bad or (first is not None and first[-1] != nF)
    return dict(verdict=CORRUPT if bad else len(head) + info["frames_bytes"], src_offsets=S, frame_offsets=[0] * (nF + 1) if bad else F,
                digests=u64s(r["digests"], r["codecs"]) if fl & DIGESTS else None, codecs=[min(int(c), 1) for c in cod[:nF]] if fl & CODECS else None,
                seg_first=first)
