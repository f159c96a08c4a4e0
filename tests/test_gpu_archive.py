"""Tensor archives on the device (FSEHIP_archive_seal_dbatch, FSEHIP_archive_open_dbatch and the Python surface around archive_tensors /
open_archive) against the numpy model of archive_corpus.py, byte for byte.  The sender compresses STRAIGHT INTO archive[head_bytes:], seals,
and the receiver inspects 64 bytes, opens and reads with the arrays the open emitted: the output must be that of the same reading call on the
loose arrays.  Every output has a mark or 0xA5 behind it, every workspace is exactly the bound.  Block-size id 0 throughout."""
import numpy as np
import pytest
import torch

import archive_corpus as ac
import planes_corpus as pc
import planes_delta_corpus as pdc
from archive_corpus import CODECS, CORRUPT, DELTA, DIGESTS, GENERIC, SPARSE, T

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, -7
M64 = (1 << 64) - 1


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def _marked(n):
    return torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")


def _filled(n, content=None):
    t = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _fields(info):
    """an ArchiveInfo as the model's fields"""
    return ac.fields(info.elemBytes, info.nTensors, info.nFrames, info.totalBytes, info.framesBytes, info.flags, info.blockSizeId, info.segLog, info.deltaOp,
                     info.sparsePermille, info.maxTotalBlocks, info.metaBytes)


class Spec:
    """one batch and how it is coded: E, the tensors (byte arrays), base (byte arrays or None) and op, seg_log (0: unsegmented), permille (None:
    dense), auto (a codec per frame, chosen), digests (ints or None), meta (bytes)"""

    def __init__(self, E, tensors, base=None, op=0, seg_log=0, permille=None, auto=False, digests=None, meta=b""):
        self.E, self.tensors, self.base, self.op, self.seg_log, self.permille, self.auto, self.digests, self.meta = E, tensors, base, op, seg_log, permille, auto, digests, meta
        self.S = pc.offsets(tensors)
        self.sizes, self.n, self.total = [len(t) for t in tensors], len(tensors), int(self.S[-1])
        self.flags = (DELTA if base is not None else 0) | (SPARSE if permille is not None else 0) | (CODECS if auto else 0) | (DIGESTS if digests is not None else 0)


def compress(hip, sp, dst=None, dst_capacity=None):
    """the compress call of the spec -> (dst, frame offsets, frame results, tensor results, codecs or None, seg_first or None)"""
    from finitestateentropy_amd.api import AutoCodec
    src = _dev(pc.cat(sp.tensors))
    base = None if sp.base is None else _dev(pc.cat(sp.base))
    first = hip.planes_segment_first(sp.sizes, sp.E, sp.seg_log) if sp.seg_log else None
    codec = AutoCodec() if sp.auto else 0
    kw = dict(block_size_id=0, dst=dst, dst_capacity=dst_capacity)
    if sp.permille is not None and sp.seg_log:
        out = hip.tensor_compress_seg_sparse_dbatch(src, sp.S, sp.E, sp.seg_log, sp.permille, first, base=base, codec=codec, delta_op=sp.op, **kw)
    elif sp.permille is not None:
        out = hip.tensor_compress_sparse_dbatch(src, sp.S, sp.E, sp.permille, base=base, codec=codec, delta_op=sp.op, **kw)
    elif sp.seg_log:
        out = hip.tensor_compress_seg_dbatch(src, sp.S, sp.E, sp.seg_log, first, base=base, codec=codec, delta_op=sp.op, **kw)
    elif sp.auto:
        out = hip.tensor_compress_mixed_dbatch(src, sp.S, sp.E, base=base, delta_op=sp.op, **kw)
    elif base is not None:
        out = hip.tensor_compress_delta_dbatch(src, base, sp.S, sp.E, codec=0, delta_op=sp.op, **kw) + (None,)
    else:
        out = hip.tensor_compress_dbatch(src, sp.S, sp.E, codec=0, **kw) + (None,)
    return out + (first,)


def decompress(hip, sp, frames, foff, soff, first, blocks, held=None):
    """the reading call of the spec over `held` (the resident bytes for a delta, in place; a marked buffer otherwise) -> (dst, results)"""
    dst = _filled(sp.total, None if sp.base is None else pc.cat(sp.base if held is None else held))
    d = dst[:max(sp.total, 1)] if sp.total == 0 else dst[:sp.total]
    base = d if sp.base is not None else None
    kw = dict(dst=d, max_total_blocks=blocks)
    if sp.permille is not None and sp.seg_log:
        res = hip.tensor_decompress_seg_sparse_dbatch(frames, foff, soff, sp.E, sp.seg_log, first, base=base, delta_op=sp.op, **kw)[1]
    elif sp.permille is not None:
        res = hip.tensor_decompress_sparse_dbatch(frames, foff, soff, sp.E, base=base, delta_op=sp.op, **kw)[1]
    elif sp.seg_log:
        res = hip.tensor_decompress_seg_dbatch(frames, foff, soff, sp.E, sp.seg_log, first, base=base, delta_op=sp.op, **kw)[1]
    elif base is not None:
        res = hip.tensor_decompress_delta_dbatch(frames, foff, base, soff, sp.E, delta_op=sp.op, **kw)[1]
    else:
        res = hip.tensor_decompress_dbatch(frames, foff, soff, sp.E, **kw)[1]
    torch.cuda.synchronize()
    return dst, res.cpu().tolist()


class Sent:
    pass


def send(hip, sp, spoil=None, short=0):
    """the sender: head_bytes from counts, compress into archive[head:], seal with a workspace of exactly the bound -> what it holds.  spoil(fres):
    changes the frame results in front of the seal; short: bytes that the capacity handed to the seal is below the archive's size"""
    x = Sent()
    first = hip.planes_segment_first(sp.sizes, sp.E, sp.seg_log) if sp.seg_log else None
    nF = int(first[-1]) if sp.seg_log else sp.n * sp.E
    x.blocks = hip.planes_block_bound(sp.total, sp.n, sp.E, 0)
    info = hip.archive_info(sp.E, sp.n, nF, sp.total, sp.flags, 0, sp.seg_log, sp.op if sp.base is not None else 0, sp.permille or 0, x.blocks, len(sp.meta))
    head = int(info.headBytes)
    assert head == ac.head_bytes(sp.n, nF, sp.flags, len(sp.meta)) and head % 256 == 0
    room = hip.frame_packed_bound(sp.total, nF, x.blocks, 0)
    x.archive = _filled(head + room)
    _, x.foff, x.fres, x.tres, x.codecs, x.first = compress(hip, sp, x.archive[head:head + room], room)
    assert (x.codecs is not None) == sp.auto
    if spoil is not None:
        spoil(x.fres)
    torch.cuda.synchronize()
    F = x.foff.cpu().tolist()
    bound = hip.archive_workspace_bound(sp.n, nF, head)
    ws = torch.full((bound + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    res = _marked(1)
    capacity = head + (room if not short else F[nF] - short)
    hip.archive_seal_dbatch(x.archive[:head + room], info, sp.S, x.foff, x.fres, x.tres, codecs=x.codecs, digests=sp.digests, meta=_dev(np.frombuffer(sp.meta, np.uint8)) if sp.meta else None,
                            capacity=capacity, result=res, workspace=ws[:bound])
    torch.cuda.synchronize()
    assert res.cpu().tolist()[1] == MARK and (ws[bound:] == FILL).all() and (x.archive[head + room:] == FILL).all(), "guards"
    x.result = res.cpu().tolist()[0]
    model, want = ac.seal(_fields(info), sp.S, F, x.fres.cpu().tolist(), x.tres.cpu().tolist(), capacity, sp.digests, None if x.codecs is None else bytes(x.codecs.cpu().numpy()),
                          sp.meta)
    got = x.archive.cpu().numpy()
    assert x.result == want, (x.result, want)
    assert (got[:head] == model).all(), np.nonzero(got[:head] != model)[0][:8]
    x.head, x.size, x.nF, x.F, x.info = head, head + F[nF], nF, F, info
    return x


def receive(hip, sp, archive, size, info=None):
    """the receiver: inspect 64 bytes, open with marked outputs and a workspace of exactly the bound -> (info, the dict of the open, the
    model's dict)"""
    if info is None:
        info = hip.archive_inspect(archive[:64].cpu().numpy(), size)
    nT, nF, E = int(info.nTensors), int(info.nFrames), int(info.elemBytes)
    bound = hip.archive_workspace_bound(nT, nF, info.headBytes)
    ws = torch.full((bound + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    outs = dict(src_offsets=_marked(nT + 1), frame_offsets=_marked(nF + 1), verdict=_marked(1))
    if info.flags & CODECS:
        outs["codecs"] = torch.full((nF + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    if info.flags & DIGESTS:
        outs["digests"] = _marked(nT)
    if info.segLog:
        outs["seg_first"] = _marked(nT * E + 1)
    got = hip.archive_open_dbatch(archive[:size], info, workspace=ws[:bound], **outs)
    torch.cuda.synchronize()
    assert (ws[bound:] == FILL).all() and all(int(outs[k][n]) == MARK for k, n in (("src_offsets", nT + 1), ("frame_offsets", nF + 1), ("verdict", 1))), "guards"
    assert "codecs" not in outs or (outs["codecs"][nF:] == FILL).all()
    assert "digests" not in outs or int(outs["digests"][nT]) == MARK
    assert "seg_first" not in outs or int(outs["seg_first"][nT * E + 1]) == MARK
    want = ac.open_(archive[:int(info.headBytes)].cpu().numpy(), _fields(info))
    have = dict(verdict=got["verdict"].cpu().tolist()[0], src_offsets=got["src_offsets"].cpu().tolist()[:nT + 1], frame_offsets=got["frame_offsets"].cpu().tolist()[:nF + 1],
                digests=None if got["digests"] is None else [d & M64 for d in got["digests"].cpu().tolist()],
                codecs=None if got["codecs"] is None else got["codecs"].cpu().tolist(), seg_first=None if got["seg_first"] is None else got["seg_first"].cpu().tolist()[:nT * E + 1])
    assert have == want, [k for k in want if have[k] != want[k]]
    return info, got, want


def round_trip(hip, sp):
    """send, receive, read with the opened arrays; the same reading call on the loose arrays of a loose compress; both equal the tensors"""
    x = send(hip, sp)
    assert x.result == x.size
    info, got, want = receive(hip, sp, x.archive, x.size)
    assert want["verdict"] == x.size and want["frame_offsets"] == x.F and want["src_offsets"] == [int(s) for s in sp.S]
    assert _fields(info) == dict(_fields(x.info), frames_bytes=x.F[x.nF]) and info.headBytes == x.head
    if sp.seg_log:
        assert want["seg_first"] == [int(f) for f in x.first]
    nT, nF = sp.n, x.nF
    opened = decompress(hip, sp, x.archive[x.head:x.size], got["frame_offsets"][:nF + 1], got["src_offsets"][:nT + 1],
                        None if got["seg_first"] is None else got["seg_first"][:nT * sp.E + 1], int(info.maxTotalBlocks))
    frames, foff, fres, tres, codecs, first = compress(hip, sp)
    torch.cuda.synchronize()
    assert foff.cpu().tolist() == x.F and torch.equal(frames[:x.F[nF]], x.archive[x.head:x.size]), "the frames in place are the loose call's"
    loose = decompress(hip, sp, frames, foff, sp.S, first, x.blocks)
    assert opened[1] == loose[1] == sp.sizes and torch.equal(opened[0], loose[0])
    back = opened[0].cpu().numpy()
    assert (back[:sp.total] == pc.cat(sp.tensors)).all() and (back[sp.total:] == FILL).all()
    return x, got


# ---------------------------------------------------------------------------------------------------------------- shapes
def _tiny_and_large(seed):
    rng = np.random.default_rng(seed)
    tiny = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in list(range(41)) + [0, 0, 1, 40, 33, 16, 17, 15, 0, 8, 24, 32, 31, 5, 0, 0, 2, 39, 40]]
    assert len(tiny) == 60
    return tiny[:30] + [pc.bf16_gaussian((3 * T + 5 + 1) // 2, seed)[:3 * T + 5]] + tiny[30:]


@pytest.mark.parametrize("E", (1, 2, 4, 8))
def test_sixty_tiny_tensors_beside_a_large_one(hip, E):
    round_trip(hip, Spec(E, _tiny_and_large(E), meta=b"x" * (E + 1)))


def test_1025_tensors_of_one_element(hip):
    sp = Spec(2, pc.random_tensors([2] * 1025, 3))
    x, _ = round_trip(hip, sp)
    assert sp.n > 1024 and x.nF == 2050


@pytest.mark.parametrize("E,seg_log,sizes", ((1, 10, [1025 * 1024 + 3, 7, 0]), (2, 11, [2 * (1024 * 2048 + 5), 10])))
def test_a_plane_of_more_than_1024_segments(hip, E, seg_log, sizes):
    tensors = [pc.bf16_gaussian((n + 1) // 2, 5 + k)[:n] for k, n in enumerate(sizes)]
    sp = Spec(E, tensors, seg_log=seg_log)
    x, _ = round_trip(hip, sp)
    counts = np.diff(np.asarray(x.first, np.int64))
    assert counts.max() > 1024 and x.nF == int(x.first[-1]) > sp.n * E


# ---------------------------------------------------------------------------------------------------------------- every kind of frames
_UPDATES = {}


def _update(E):
    """(old, new, stale): bf16 (E == 2) or fp32 (E == 4) weights of T, 2 T + 5 and T - 3 elements, an update step, and `old` with one element
    of tensor 1 changed"""
    if E not in _UPDATES:
        counts = [T, 2 * T + 5, T - 3]
        w = np.random.default_rng(1).normal(0, 0.02, sum(counts)).astype(np.float32)
        w2 = (w + np.random.default_rng(2).normal(0, 2e-5, sum(counts))).astype(np.float32)
        old, new = (pdc.bf16_bytes(x) if E == 2 else x.view(np.uint8) for x in (w, w2))
        cuts = [E * int(c) for c in np.concatenate([[0], np.cumsum(counts)])]
        old, new = ([np.ascontiguousarray(x[a:b]) for a, b in zip(cuts, cuts[1:])] for x in (old, new))
        stale = [o.copy() for o in old]
        stale[1][150 * E + E - 1] ^= 0x01
        _UPDATES[E] = (old, new, stale)
    return _UPDATES[E]


KINDS = {"plain": dict(), "xor": dict(delta=True, op=0), "sub": dict(delta=True, op=1), "segmented": dict(delta=True, op=1, seg_log=10),
         "sparse": dict(delta=True, op=1, permille=500), "sparse segmented": dict(delta=True, op=1, permille=500, seg_log=11),
         "codec per frame": dict(delta=True, op=1, auto=True), "codec per segment": dict(seg_log=10, auto=True)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_round_trip_of_every_kind(hip, kind):
    k = dict(KINDS[kind])
    old, new, _ = _update(2)
    sp = Spec(2, new, base=old if k.pop("delta", False) else None, meta=kind.encode(), **k)
    x, got = round_trip(hip, sp)
    f = ac.header_fields(x.archive[:64].cpu().numpy())
    assert (f["seg_log"], f["delta_op"], f["sparse_permille"], f["flags"]) == (sp.seg_log, sp.op if sp.base is not None else 0, sp.permille or 0, sp.flags)
    assert ac.parse(x.archive[:x.head].cpu().numpy())[5] == kind.encode()


@pytest.mark.parametrize("E", (2, 4))
def test_checked_delta_through_an_archive_the_gate_fed_from_the_opened_digests(hip, E):
    old, new, stale = _update(E)
    S = pc.offsets(old)
    expected = [d & M64 for d in hip.tensor_digest_dbatch(_dev(pc.cat(old)), S)[0].cpu().tolist()]
    sp = Spec(E, new, base=old, op=1, seg_log=10, digests=expected)
    x, got = round_trip(hip, sp)
    n, nF = sp.n, x.nF
    first, foff, soff = got["seg_first"][:n * E + 1], got["frame_offsets"][:nF + 1], got["src_offsets"][:n + 1]
    for held, verdict, want in ((old, sp.sizes, new), (stale, [sp.sizes[0], CORRUPT, sp.sizes[2]], [new[0], stale[1], new[2]])):
        dst = _filled(sp.total, pc.cat(held))
        dig, res = hip.tensor_digest_dbatch(dst[:sp.total], soff)
        G, R = hip.tensor_gate_dbatch(foff, dig, res, got["digests"], E, frame_first=first)
        assert R.cpu().tolist() == verdict
        res = hip.tensor_decompress_seg_dbatch(x.archive[x.head:x.size], G, soff, E, 10, first, base=dst[:sp.total], dst=dst[:sp.total], max_total_blocks=x.blocks, delta_op=1)[1]
        torch.cuda.synchronize()
        assert [r if v >= 0 else (r < 0) for r, v in zip(res.cpu().tolist(), verdict)] == [v if v >= 0 else True for v in verdict]
        back = dst.cpu().numpy()
        assert (back[:sp.total] == pc.cat(want)).all() and (back[sp.total:] == FILL).all()


def test_window_read_and_patch_on_an_opened_segmented_archive(hip):
    E, L = 2, 10
    old, new, _ = _update(E)
    sp = Spec(E, old, seg_log=L)
    x, got = round_trip(hip, sp)
    n, nF = sp.n, x.nF
    frames = x.archive[x.head:x.size]
    first, foff, soff = got["seg_first"][:n * E + 1], got["frame_offsets"][:nF + 1], got["src_offsets"][:n + 1]
    wins = [(100, 300), (0, 0), (T - 600, T - 3)]
    D = np.concatenate([[0], np.cumsum([E * (b - a) for a, b in wins])]).astype(np.uint64)
    dst, res = hip.tensor_decompress_window_dbatch(frames, foff, sp.S, wins, D, E, L, first.cpu().numpy().astype(np.uint64), block_size_id=0)
    torch.cuda.synchronize()
    want = pc.cat([t[E * a:E * b] for t, (a, b) in zip(old, wins)])
    assert res.cpu().tolist() == [E * (b - a) for a, b in wins] and (dst.cpu().numpy()[:len(want)] == want).all()
    # the patch: the frame results of an opened archive are the extents of its offsets
    cur = [o.copy() for o in old]
    for t, u, (a, b) in zip(cur, new, wins):
        t[E * a:E * b] = u[E * a:E * b]
    fres = foff[1:] - foff[:-1]
    out, ooff, ores, tres, _ = hip.tensor_patch_window_dbatch(frames, foff, fres, _dev(pc.cat(cur)), sp.S, wins, E, L, first.cpu().numpy().astype(np.uint64), block_size_id=0)
    torch.cuda.synchronize()
    whole = compress(hip, Spec(E, cur, seg_log=L))
    torch.cuda.synchronize()
    end = int(whole[1][-1])
    assert tres.cpu().tolist() == sp.sizes and ooff.cpu().tolist() == whole[1].cpu().tolist() and torch.equal(out[:end], whole[0][:end])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_seal_refuses_a_failed_frame_and_a_short_capacity(hip):
    old, new, _ = _update(2)
    sp = Spec(2, new, base=old, op=1, meta=b"m")

    def spoil(fres):
        fres[3] = -4
    for kw, want in ((dict(spoil=spoil), GENERIC), (dict(short=1), ac.TOO_SMALL)):
        x = send(hip, sp, **kw)                                                      # (compares the head with the model's, whose magic is 0)
        assert x.result == want and not x.archive[:4].cpu().numpy().any(), kw
        with pytest.raises(ValueError, match="GENERIC"):
            hip.archive_inspect(x.archive[:64].cpu().numpy(), x.size)
    assert send(hip, sp, short=0).result > 0


def test_open_refuses_every_damage_and_the_resident_tensors_stay(hip):
    E, L = 2, 10
    old, new, _ = _update(E)
    S = pc.offsets(old)
    expected = [d & M64 for d in hip.tensor_digest_dbatch(_dev(pc.cat(old)), S)[0].cpu().tolist()]
    sp = Spec(E, new, base=old, op=1, seg_log=L, auto=True, digests=expected, meta=b"meta!")
    x = send(hip, sp)
    good = x.archive[:x.size].cpu().numpy()
    head, n, nF = x.head, sp.n, x.nF
    r = ac.regions(n, nF, sp.flags, len(sp.meta))
    assert r["pad"] + 8 < head - 8, "there is padding to damage"
    resident = pc.cat(old)

    def flip(at, bit=0):
        def f(h):
            h[at] ^= 1 << bit
        return f

    def u64(at, value):
        def f(h):
            h[at:at + 8] = np.array([value], "<u8").view(np.uint8)
        return f

    def swap(a, b):
        def f(h):
            t = h[a:a + 8].copy()
            h[a:a + 8] = h[b:b + 8]
            h[b:b + 8] = t
        return f
    F = x.F
    k = next(q for q in range(1, nF - 1) if F[q] < F[q + 1])
    cases = []
    for name, a, b in (("sizes", r["sizes"], r["offsets"]), ("offsets", r["offsets"], r["digests"]), ("digests", r["digests"], r["codecs"])):
        cases += [("bit in the first of the " + name, flip(a + 1, 3), False), ("bit in the last of the " + name, flip(b - 8 + 2, 5), False)]
    cases += [("bit in the first codec", flip(r["codecs"]), False), ("bit in the last codec", flip(r["codecs"] + nF - 1), False),
              ("bit in the meta", flip(r["meta"] + 2, 6), False), ("bit in the padding", flip(r["pad"] + 9, 4), False), ("bit in the digest", flip(head - 3, 7), False),
              ("bit in the header", flip(41), False)]
    # behind a digest re-stamped with the model: the field checks themselves
    cases += [("first offset not 0", u64(r["offsets"], 1), True), ("offsets that decrease", swap(r["offsets"] + 8 * k, r["offsets"] + 8 * (k + 1)), True),
              ("last offset not framesBytes", u64(r["digests"] - 8, F[nF] - 1), True), ("size sum off by one", u64(r["sizes"] + 8, sp.sizes[1] + 1), True),
              ("size sum off by one the other way", u64(r["sizes"], sp.sizes[0] - 1), True), ("a size above totalBytes", u64(r["sizes"] + 16, sp.total + 1), True),
              ("codec byte 2", lambda h: h.__setitem__(r["codecs"] + 1, 2), True), ("codec padding", lambda h: h.__setitem__(r["codecs"] + nF, 1), True),
              ("meta padding", lambda h: h.__setitem__(r["meta"] + len(sp.meta), 1), True), ("padding", lambda h: h.__setitem__(head - 9, 0x80), True),
              ("segLog the frames were not cut by", lambda h: h.__setitem__(10, L + 1), True)]
    for name, damage, stamp in cases:
        bad = good.copy()
        damage(bad[:head])
        if stamp:
            ac.restamp(bad[:head])
        info = hip.archive_inspect(bad[:64] if name.startswith("segLog") else good[:64], x.size)
        archive = _filled(x.size, bad)
        _, got, want = receive(hip, sp, archive, x.size, info)                       # (equal to the model's open, guards checked)
        assert want["verdict"] == CORRUPT and want["frame_offsets"] == [0] * (nF + 1), name
        dst = _filled(sp.total, resident)
        # (the receiver reads with its own segFirst: the refused open's is that of the sizes it found, clamped)
        res = hip.tensor_decompress_seg_dbatch(archive[head:x.size], got["frame_offsets"][:nF + 1], S, E, L, x.first, base=dst[:sp.total], dst=dst[:sp.total],
                                               max_total_blocks=x.blocks, delta_op=1)[1]
        torch.cuda.synchronize()
        assert all(v < 0 for v in res.cpu().tolist()), name
        back = dst.cpu().numpy()
        assert (back[:sp.total] == resident).all() and (back[sp.total:] == FILL).all(), name
    # a header that differs from the info: the archive is intact, the receiver's copy of a field is not
    for field, value in (("maxTotalBlocks", x.blocks + 1), ("totalBytes", sp.total - 1), ("sparsePermille", 0), ("framesBytes", F[nF] - 1)):
        info = hip.archive_inspect(good[:64], x.size)
        if field == "sparsePermille":
            info.flags, value = info.flags | SPARSE, 7
        setattr(info, field, value)
        _, got, want = receive(hip, sp, _filled(x.size, good), x.size, info)
        assert want["verdict"] == CORRUPT and want["frame_offsets"] == [0] * (nF + 1), field
    # and undamaged it opens
    assert receive(hip, sp, _filled(x.size, good), x.size)[2]["verdict"] == x.size


# ---------------------------------------------------------------------------------------------------------------- one graph
def test_compress_seal_open_and_decompress_in_one_hip_graph(hip):
    """one captured graph on a single stream: compress into the archive, seal, open, decompress.  The receiver's info holds framesBytes, so a
    replay opens only an archive of the size the graph was captured with: the sources are incompressible (every block is stored raw, the
    frames' total does not depend on the bytes), replayed over changed bytes; a last replay over a source that compresses is refused by the
    open inside the graph -- its header is not the info's -- and the destination keeps its bytes."""
    import ctypes as C
    E = 2
    sizes = [2 * T + 6, 10, 0, T - 2]
    first_src, second_src, other = pc.random_tensors(sizes, 11), pc.random_tensors(sizes, 12), [pc.bf16_gaussian((n + 1) // 2, 9)[:n] for n in sizes]
    sp = Spec(E, first_src, meta=b"graph")
    x = send(hip, sp)                                                                 # an ordinary pass: framesBytes for the receiver's info
    info_w = x.info
    info_r = hip.archive_inspect(x.archive[:64].cpu().numpy(), x.size)
    n, nF, head, total = sp.n, x.nF, x.head, sp.total
    room = hip.frame_packed_bound(total, nF, x.blocks, 0)
    src, archive, dst, planes, planes2 = _filled(total), _filled(head + room), _filled(total), _filled(total), _filled(total)
    soff = torch.from_numpy(sp.S.astype(np.int64)).cuda()
    foff, poff, ofoff, poff2 = (torch.zeros(nF + 1, dtype=torch.int64, device="cuda") for _ in range(4))
    fres, pres = (torch.zeros(nF, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    osoff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    sres, verdict = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    meta = _dev(np.frombuffer(sp.meta, np.uint8))
    wsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize
    wsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(nF), C.c_size_t(x.blocks), C.c_uint(0), C.c_int(0))), dtype=torch.uint8, device="cuda")
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t
    rws = torch.empty(int(rsize(C.c_size_t(nF), C.c_size_t(x.blocks))), dtype=torch.uint8, device="cuda")
    aws = torch.empty(hip.archive_workspace_bound(n, nF, head), dtype=torch.uint8, device="cuda")

    def work():
        hip.tensor_compress_dbatch(src[:total], soff, E, 0, 0, capacity=total, dst=archive[head:head + room], dst_capacity=room, max_total_blocks=x.blocks,
                                   frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes[:total], plane_offsets=poff, workspace=wws)
        hip.archive_seal_dbatch(archive[:head + room], info_w, soff, foff, fres, tres, meta=meta, result=sres, workspace=aws)
        hip.archive_open_dbatch(archive[:x.size], info_r, src_offsets=osoff, frame_offsets=ofoff, verdict=verdict, workspace=aws)
        hip.tensor_decompress_dbatch(archive[head:x.size], ofoff, osoff, E, dst=dst[:total], dst_capacity=total, max_total_blocks=x.blocks, planes=planes2[:total],
                                     planes_capacity=total, plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres)
    src[:total] = _dev(pc.cat(first_src)); work(); torch.cuda.synchronize()           # one ordinary call first
    assert (dst.cpu().numpy()[:total] == pc.cat(first_src)).all() and int(verdict[0]) == x.size
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for tensors, opens in ((second_src, True), (first_src, True), (other, False)):
        src[:total] = _dev(pc.cat(tensors))
        before = dst.cpu().numpy().copy()
        for t in (sres, verdict, rres, ofoff, osoff):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        back = dst.cpu().numpy()
        if opens:
            assert int(sres[0]) == int(verdict[0]) == x.size and rres.cpu().tolist() == sizes
            assert (back[:total] == pc.cat(tensors)).all() and (back[total:] == FILL).all()
            assert (archive.cpu().numpy()[:head] == ac.seal(_fields(info_w), sp.S, foff.cpu().tolist(), fres.cpu().tolist(), tres.cpu().tolist(), head + room, None, None, sp.meta)[0]).all()
        else:
            assert 0 < int(sres[0]) != x.size and int(verdict[0]) == CORRUPT and not ofoff.cpu().numpy().any()
            assert all(v < 0 for v, s in zip(rres.cpu().tolist(), sizes) if s) and (back == before).all()


# ---------------------------------------------------------------------------------------------------------------- Python
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.fixture(scope="module")
def mixed():
    gen = torch.Generator(device="cuda").manual_seed(13)
    old_np, new_np = pdc.bf16_update_pair(1 << 16)
    old = [torch.from_numpy(old_np.copy()).cuda().view(torch.bfloat16).reshape(256, 256), torch.randn((1000, 3), generator=gen, device="cuda") * 0.02,
           torch.randn((T // 4 + 3,), generator=gen, device="cuda") * 0.02, torch.arange(77, device="cuda", dtype=torch.uint8),
           torch.arange(-50, 50, device="cuda", dtype=torch.int64), torch.zeros((0, 4), device="cuda", dtype=torch.float16)]
    new = [torch.from_numpy(new_np.copy()).cuda().view(torch.bfloat16).reshape(256, 256), old[1] + 1e-5, old[2] * 1.0001, old[3] + 1, old[4] + 3, old[5].clone()]
    return old, new


def test_save_and_load_on_mixed_dtypes(hip, mixed, tmp_path):
    import finitestateentropy_amd
    from finitestateentropy_amd.api import AutoCodec
    _, new = mixed
    for obj in (hip.compress_tensors(new, codec=AutoCodec(5)), hip.compress_tensors_segmented(new, segment_log=15, codec=1), hip.compress_tensors([])):
        path = str(tmp_path / "update.fsta")
        nbytes = hip.save_tensors(obj, path)
        buf = hip.archive_tensors(obj)
        assert nbytes == buf.numel() and nbytes % 256 == 0 and buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_cuda
        back = finitestateentropy_amd.load_tensors(path)
        assert (back.codec, back.block_size_id, back.segment_log, back.delta, back.sparse_permille, back.base_digests) == \
            (obj.codec, obj.block_size_id, obj.segment_log, False, None, None)
        assert back.dtypes == obj.dtypes and back.shapes == obj.shapes and len(back.groups) == len(obj.groups)
        for a, b in zip(back.groups, obj.groups):
            assert a["elem_bytes"] == b["elem_bytes"] and a["index"] == b["index"] and a["sizes"] == b["sizes"] and torch.equal(a["frames"], b["frames"])
            assert torch.equal(a["frame_offsets"], b["frame_offsets"]) and ("codecs" in a) == ("codecs" in b) and ("seg_first" in a) == ("seg_first" in b)
        out = hip.decompress_tensors(back)
        assert len(out) == len(obj.dtypes) and all(_same(a, b) for a, b in zip(out, new))
    obj = hip.compress_tensors_segmented(new, segment_log=15)
    win = [None, None, (5, 900), None, None, None]
    assert _same(hip.decompress_tensor_windows(hip.open_archive(hip.archive_tensors(obj).cpu().numpy()), win)[2], new[2].reshape(-1)[5:900]), "host bytes are uploaded"


def test_checked_sparse_delta_through_open_archive(hip, mixed):
    from finitestateentropy_amd.api import DeltaBase, SparsePlanes
    old, new = mixed
    obj = hip.compress_tensors(new, codec=SparsePlanes(1), base=DeltaBase(old, "sub", check=True))
    buf = hip.archive_tensors(obj)
    back = hip.open_archive(buf)
    assert (back.delta, back.delta_op, back.sparse_permille, back.codec, back.base_digests) == (True, "sub", 500, SparsePlanes(1), obj.base_digests)
    assert all(g["frames"].data_ptr() >= buf.data_ptr() and g["frames"].data_ptr() < buf.data_ptr() + buf.numel() for g in back.groups if g["frames"].numel()), "views"
    out = hip.decompress_tensors(back, base=DeltaBase(old, "sub"))
    assert all(_same(a, b) for a, b in zip(out, new))
    stale = [t.clone() for t in old]
    stale[2][7] += 1.0
    with pytest.raises(ValueError, match=r"tensors \[2\]"):
        hip.decompress_tensors(back, base=stale)
    # damage: a byte of the second archive's index, a header field, a cut buffer -- ValueError says where
    second = next(at for at in range(256, buf.numel(), 256) if bytes(buf[at:at + 4].cpu().numpy()) == ac.MAGIC)
    for at, what in ((second + 70, "archive 1 .* refused on the device"), (9, "archive 0 .*header refused"), (second + 5, "archive 1 .*header refused")):
        bad = buf.clone()
        bad[at] ^= 0x40
        with pytest.raises(ValueError, match=what):
            hip.open_archive(bad)
    with pytest.raises(ValueError, match="srcSize_wrong"):
        hip.open_archive(buf[:buf.numel() - 256])
