"""The packed frame writer with a codec per frame (FSEHIP_frame_compress_packed_mixed_dbatch: GIVEN by the caller, or chosen by size) and the
tensor composite on top of it, against the CPU oracle's frames (checker.frame_compress of every content with either codec) and the integer
rule of frame_mixed_corpus.expected_choice -- never against a choice the library made.  The only comparison with the library itself is the
one the contract states: all codecs 0 (or 1) is the existing packed writer, bit for bit.  Every destination is filled with 0xA5 and has a
tail behind it: whatever is not a byte of a frame that succeeded must still be 0xA5.  The binding's guard mode is on (conftest.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_delta_corpus as pdc
from frame_mixed_corpus import GENERIC, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
GIVEN, CHOOSE = 0, 1
SZ, VP = C.c_size_t, C.c_void_p


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _filled(n):
    return torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")


def _blocks(contents, bsid):
    return sum(fmc.block_count(len(c), bsid) for c in contents)


def _corpus(oracle, bsid):
    """(contents, the oracle's FSE frames, its Huff0 frames)"""
    return [c for _, c in fmc.contents(oracle)], fmc.frames(oracle, bsid, 0), fmc.frames(oracle, bsid, 1)


def write(hip, contents, codecs, tol=0, bsid=0, align_log=0, cap=None, room=None, promise=None):
    """one call (codecs a list: GIVEN; None: CHOOSE at `tol`) into `room` bytes of FILL (default: the capacity, whose default is
    FSEHIP_frame_packedBound) with a tail of FILL behind them: -> (results, offsets, every byte of the destination, codecs)"""
    n = len(contents)
    if cap is None:
        cap = hip.frame_packed_bound(sum(len(c) for c in contents), n, _blocks(contents, bsid), align_log)
    dst = _filled(cap if room is None else room)
    given = None if codecs is None else _dev(np.asarray(codecs, np.uint8))
    _, doff, res, got = hip.frame_compress_packed_mixed_dbatch(_dev(pc.cat(contents)), pc.offsets(contents), given, tol, bsid, dst=dst, capacity=cap,
                                                               max_total_blocks=_blocks(contents, bsid) if promise is None else promise, align_log=align_log)
    return res.cpu().tolist(), doff.cpu().tolist(), dst.cpu().numpy(), got.cpu().tolist()


def check(want, res, off, out, align_log, cap, what):
    """want[i]: the oracle's frame of content i, or the (negative) error the frame ends with whatever the capacity"""
    sizes = [w if isinstance(w, int) else len(w) for w in want]
    assert off == fpc.packed_offsets(sizes, align_log, cap), what
    assert res == fpc.packed_results(sizes, align_log, cap), what
    written = np.zeros(len(out), bool)
    for i, w in enumerate(want):
        if res[i] > 0:
            assert (out[off[i]:off[i] + res[i]] == w).all(), (what, i)
            written[off[i]:off[i] + res[i]] = True
    assert (out[~written] == FILL).all(), (what, "bytes outside the frames", np.nonzero((out != FILL) & ~written)[0][:8])


def pick(F, H, codecs):
    return [H[i] if c == 1 else F[i] if c == 0 else GENERIC for i, c in enumerate(codecs)]


def raw(hip, dst, cap, doff, res, src, soff, n, nblk, bsid, codecs, policy, tol, align_log, ws):
    """FSEHIP_frame_compress_packed_mixed_dbatch itself (dst None: a NULL destination): -> its return value"""
    return hip.lib.FSEHIP_frame_compress_packed_mixed_dbatch(VP(dst.data_ptr() if dst is not None else 0), C.c_uint64(cap), VP(doff.data_ptr()), VP(res.data_ptr()),
                                                             VP(src.data_ptr()), VP(soff.data_ptr()), SZ(n), SZ(nblk), C.c_uint(bsid), VP(codecs.data_ptr()), C.c_int(policy),
                                                             C.c_uint(tol), C.c_uint(align_log), VP(ws.data_ptr()), SZ(ws.numel()), VP(torch.cuda.current_stream().cuda_stream))


# ---------------------------------------------------------------------------------------------------------------- GIVEN
@pytest.mark.parametrize("align_log", [0, 4])
@pytest.mark.parametrize("bsid", fmc.BSIDS)
def test_given_codecs_give_the_oracles_frame_of_each_codec(hip, checker, bsid, align_log):
    contents, F, H = _corpus(checker, bsid)
    n = len(contents)
    if bsid == 0:
        assert _blocks(contents, 0) > 64 and fmc.block_count(len(contents[7]), 0) == 5
    for codecs in ([i & 1 for i in range(n)], [1 - (i & 1) for i in range(n)]):
        res, off, out, got = write(hip, contents, codecs, bsid=bsid, align_log=align_log)
        check(pick(F, H, codecs), res, off, out, align_log, fpc.NO_CAP, (bsid, align_log, codecs))
        assert got == codecs, "an input: returned as it is"
    for codec in (0, 1):                                     # all of one codec: the existing packed writer, bit for bit
        res, off, out, _ = write(hip, contents, [codec] * n, bsid=bsid, align_log=align_log)
        check((F, H)[codec], res, off, out, align_log, fpc.NO_CAP, (bsid, align_log, "all", codec))
        dst = _filled(len(out) - TAIL)
        _, doff, pres = hip.frame_compress_packed_dbatch(_dev(pc.cat(contents)), pc.offsets(contents), bsid, codec, dst=dst, capacity=len(out) - TAIL,
                                                         max_total_blocks=_blocks(contents, bsid), align_log=align_log)
        assert doff.cpu().tolist() == off and pres.cpu().tolist() == res and (dst.cpu().numpy() == out).all()


def test_given_codec_bytes_that_name_no_coder(hip, checker):
    contents, F, H = _corpus(checker, 0)
    n = len(contents)
    codecs = [i & 1 for i in range(n)]
    codecs[3], codecs[7], codecs[n - 1] = 2, 255, 2          # the RLE content, the five-block P80 content, the last frame
    res, off, out, _ = write(hip, contents, codecs, align_log=4)
    check(pick(F, H, codecs), res, off, out, 4, fpc.NO_CAP, "codec bytes 2 and 255")
    for i in (3, 7, n - 1):
        assert res[i] == GENERIC and off[i + 1] == off[i], "GENERIC, and no room taken"
    assert res[2] == len(F[2]) and res[4] == len(F[4]) and res[6] == len(F[6]) and res[8] == len(F[8])


# ---------------------------------------------------------------------------------------------------------------- CHOOSE
@pytest.mark.parametrize("tol", fmc.TOLERANCES)
@pytest.mark.parametrize("bsid", fmc.BSIDS)
def test_choose_follows_the_rule_on_the_oracles_sizes(hip, checker, bsid, tol):
    contents, F, H = _corpus(checker, bsid)
    want = fmc.choices(checker, bsid, tol)
    if tol in (0, 50):
        assert set(want) == {0, 1}
    align_log = 4 if tol == 20 else 0
    res, off, out, got = write(hip, contents, None, tol, bsid=bsid, align_log=align_log)
    print("block-size id %d, tolerance %d: FSE %s Huff0 %s -> %s" % (bsid, tol, [len(f) for f in F], [len(h) for h in H], got))
    assert got == want
    check(pick(F, H, want), res, off, out, align_log, fpc.NO_CAP, (bsid, tol))
    # ... and the frames are the GIVEN frames of the choice, in the same places
    res2, off2, out2, _ = write(hip, contents, got, bsid=bsid, align_log=align_log)
    assert res2 == res and off2 == off and (out2 == out).all()


@pytest.mark.parametrize("policy", [GIVEN, CHOOSE])
def test_promise_one_block_short(hip, checker, policy):
    contents, F, H = _corpus(checker, 0)
    n = len(contents)
    want = fmc.choices(checker, 0, 50) if policy == CHOOSE else [1 - (i & 1) for i in range(n)]
    assert len(contents[-1]) > 0
    res, off, out, got = write(hip, contents, None if policy == CHOOSE else want, 50, align_log=4, promise=_blocks(contents, 0) - 1)
    check(pick(F, H, want)[:n - 1] + [GENERIC], res, off, out, 4, fpc.NO_CAP, "promise short")
    assert res[n - 1] == GENERIC and off[n] == off[n - 1], "the last frame, and it takes no room"
    assert got == (want[:n - 1] + [0] if policy == CHOOSE else want), "both trials fail: codec 0"
    # no promise at all: empty contents still give their 8-byte frames (Huff0 under CHOOSE: a tie)
    few = [np.zeros(0, np.uint8), np.array([1], np.uint8), np.zeros(0, np.uint8)]
    res, off, out, got = write(hip, few, None if policy == CHOOSE else [0, 1, 1], 0, promise=0)
    kind = [1, 0, 1] if policy == CHOOSE else [0, 1, 1]
    check([(F, H)[kind[0]][0], GENERIC, (F, H)[kind[2]][0]], res, off, out, 0, fpc.NO_CAP, "promise 0")
    assert res == [8, GENERIC, 8] and off == [0, 8, 8, 16] and got == kind


@pytest.mark.parametrize("policy", [GIVEN, CHOOSE])
def test_capacity_that_cuts_the_last_frame(hip, checker, policy):
    contents, F, H = _corpus(checker, 0)
    n = len(contents)
    want = fmc.choices(checker, 0, 0) if policy == CHOOSE else [i & 1 for i in range(n)]
    frames = pick(F, H, want)
    U = fpc.packed_offsets([len(f) for f in frames], 0)
    codecs = None if policy == CHOOSE else want
    full, off_full, out_full, got_full = write(hip, contents, codecs, cap=U[n])
    check(frames, full, off_full, out_full, 0, U[n], "exact capacity")
    assert full == [len(f) for f in frames] and got_full == want
    res, off, out, got = write(hip, contents, codecs, cap=U[n] - 1, room=U[n])
    check(frames, res, off, out, 0, U[n] - 1, "one short")
    assert res[:n - 1] == full[:n - 1] and res[n - 1] == TOO_SMALL and got == want, "the choice does not depend on the capacity"
    assert (out[:U[n - 1]] == out_full[:U[n - 1]]).all() and (out[U[n - 1]:] == FILL).all()
    k = 6                                                    # the capacity ends 5 bytes into an earlier frame
    res, off, out, got = write(hip, contents, codecs, cap=U[k] + 5, room=U[n])
    check(frames, res, off, out, 0, U[k] + 5, "inside frame %d" % k)
    assert res[k:] == [TOO_SMALL] * (n - k) and got == want and (out[U[k]:] == FILL).all()


@pytest.mark.parametrize("policy", [GIVEN, CHOOSE])
def test_sizing_query_no_frames_and_the_codec_bytes(hip, checker, policy):
    contents, F, H = _corpus(checker, 0)
    n, nblk = len(contents), _blocks(contents, 0)
    want = fmc.choices(checker, 0, 20) if policy == CHOOSE else [i & 1 for i in range(n)]
    sizes = [len(f) for f in pick(F, H, want)]
    src, soff = _dev(pc.cat(contents)), _i64(pc.offsets(contents))
    need = hip.frame_mixed_workspace_bound(n, nblk, 0, choose=policy == CHOOSE)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def fresh():
        codecs = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
        if policy == GIVEN:
            codecs[:n] = _dev(np.asarray(want, np.uint8))
        return torch.full((n + 2,), -7, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -7, dtype=torch.int64, device="cuda"), codecs
    for align_log in (0, 4):
        doff, res, codecs = fresh()
        assert raw(hip, None, (1 << 64) - 1, doff, res, src, soff, n, nblk, 0, codecs, policy, 20, align_log, ws) == 0     # d_dst NULL, UINT64_MAX
        torch.cuda.synchronize()
        assert doff.cpu().tolist() == fpc.packed_offsets(sizes, align_log) + [-7] and res.cpu().tolist() == sizes + [-7]
        assert codecs.cpu().tolist() == want + [7] * 8, "n bytes of the codecs, no other"
        cap = int(doff[n])
        dst = _filled(cap)
        doff2, res2, codecs2 = fresh()
        assert raw(hip, dst, cap, doff2, res2, src, soff, n, nblk, 0, codecs2, policy, 20, align_log, ws) == 0
        torch.cuda.synchronize()
        assert torch.equal(doff2, doff) and torch.equal(res2, res) and torch.equal(codecs2, codecs)
        check(pick(F, H, want), res2.cpu().tolist()[:n], doff2.cpu().tolist()[:n + 1], dst.cpu().numpy(), align_log, cap, "at the queried capacity")
    # a workspace one byte short, then no frames: entry 0 of the offsets and nothing else
    doff, res, codecs = fresh()
    dst = _filled(64)
    assert raw(hip, dst, 64, doff, res, src, soff, n, nblk, 0, codecs, policy, 20, 0, ws[:need - 1]) == 1
    assert raw(hip, dst, 64, doff, res, src, soff, 0, nblk, 0, codecs, policy, 20, 0, ws) == 0
    torch.cuda.synchronize()
    assert doff.cpu().tolist() == [0] + [-7] * (n + 1) and bool((res == -7).all()) and bool((dst == FILL).all())
    assert codecs.cpu().tolist()[n:] == [7] * 8 and (policy == GIVEN or codecs.cpu().tolist()[:n] == [7] * n)
    # the binding on its own: destination, workspace and (CHOOSE) codecs of its own, all guarded in guard mode
    dst3, doff3, res3, got3 = hip.frame_compress_packed_mixed_dbatch(src, pc.offsets(contents), None if policy == CHOOSE else _dev(np.asarray(want, np.uint8)), 20, 0)
    assert got3.cpu().tolist() == want and res3.cpu().tolist() == sizes and doff3.cpu().tolist() == fpc.packed_offsets(sizes, 0)
    e = hip.frame_compress_packed_mixed_dbatch(src[:0], np.zeros(1, np.uint64), None if policy == CHOOSE else src[:0], 0, 0)
    assert e[1].cpu().tolist() == [0] and e[2].numel() == 0 and e[3].numel() == 0


# ---------------------------------------------------------------------------------------------------------------- reading
@pytest.mark.parametrize("bsid", fmc.BSIDS)
def test_mixed_frames_through_the_packed_reader(hip, checker, bsid):
    contents, _, _ = _corpus(checker, bsid)
    n, total = len(contents), sum(len(c) for c in contents)
    src = _dev(pc.cat(contents))
    frames, foff, fres, codecs = hip.frame_compress_packed_mixed_dbatch(src, pc.offsets(contents), None, 50, bsid, align_log=4)
    assert set(codecs.cpu().tolist()) == {0, 1}
    magics = [int.from_bytes(frames[int(o):int(o) + 4].cpu().numpy().tobytes(), "little") for o in foff.cpu().tolist()[:n]]
    assert magics == [0x183E3309 if c else 0x183E2309 for c in codecs.cpu().tolist()], "every frame says which coder wrote it"
    back, boff, bres = hip.frame_decompress_packed_dbatch(frames, foff, capacity=total, max_total_blocks=_blocks(contents, bsid))
    assert bres.cpu().tolist() == [len(c) for c in contents] and boff.cpu().tolist() == [int(x) for x in pc.offsets(contents)]
    assert (back.cpu().numpy()[:total] == pc.cat(contents)).all()


# ---------------------------------------------------------------------------------------------------------------- the tensor composite
def _tensors(E):
    """tensors and bases of E-byte elements: the bf16 update cut to 24 KB (as E-byte elements it is still its bytes), random against random, an
    unchanged tensor (sparse: a byte in sixteen is not zero), an empty one, and a size that is no multiple of E"""
    rng = np.random.default_rng(500 + E)
    old, new = pdc.bf16_update_pair(1 << 14)
    same = (rng.integers(1, 256, 700 * E, dtype=np.uint8) * (rng.integers(0, 16, 700 * E) == 0)).astype(np.uint8)      # sparse: FSE's by far, also in the plain form
    odd_base = rng.integers(0, 256, 600 * E + E - 1, dtype=np.uint8)
    odd = odd_base ^ (rng.integers(1, 256, odd_base.size, dtype=np.uint8) * (rng.integers(0, 16, odd_base.size) == 0)).astype(np.uint8)
    tensors = [new[:24 << 10], rng.integers(0, 256, 1025 * E, dtype=np.uint8), same, np.zeros(0, np.uint8), odd]
    bases = [old[:24 << 10], rng.integers(0, 256, 1025 * E, dtype=np.uint8), same.copy(), np.zeros(0, np.uint8), odd_base]
    return tensors, bases


def _plane_frames(checker, tensors, E, capacity=None):
    """per plane of every tensor the oracle's (FSE frame, Huff0 frame); a refused tensor's planes are empty contents"""
    S = [int(x) for x in pc.offsets(tensors)]
    out = []
    for i, t in enumerate(tensors):
        refused = capacity is not None and S[i + 1] > capacity
        for pl in pc.planes_of(t, E):
            data = np.zeros(0, np.uint8) if refused else np.ascontiguousarray(pl)
            out.append(tuple(f[:r].copy() for r, f in (checker.frame_compress(data, 0, c) for c in (0, 1))))
    return out


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("E", [2, 4])
def test_tensor_composite_given_chosen_refused_and_read_back(hip, checker, E, delta):
    tensors, bases = _tensors(E)
    n, S = len(tensors), [int(x) for x in pc.offsets(tensors)]
    total = S[-1]
    coded = pdc.xor_all(tensors, bases) if delta else tensors
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, 4)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))

    def run(codecs, tol=0, capacity=None):
        dst = _filled(fcap)
        given = None if codecs is None else _dev(np.asarray(codecs, np.uint8))
        _, foff, fres, tres, got = hip.tensor_compress_mixed_dbatch(src, pc.offsets(tensors), E, base if delta else None, given, tol, 0, capacity=capacity, dst=dst,
                                                                    dst_capacity=fcap, max_total_blocks=blocks, align_log=4)
        return dst, foff, fres, tres.cpu().tolist(), got.cpu().tolist()
    pairs = _plane_frames(checker, coded, E)
    F, H = [p[0] for p in pairs], [p[1] for p in pairs]
    # GIVEN with a pattern per plane: the low plane Huff0, every other plane FSE
    pattern = [1 if p == 0 else 0 for _ in range(n) for p in range(E)]
    dst, foff, fres, tres, got = run(pattern)
    check(pick(F, H, pattern), fres.cpu().tolist(), foff.cpu().tolist(), dst.cpu().numpy(), 4, fcap, ("given", E, delta))
    assert tres == [len(t) for t in tensors] and got == pattern
    # CHOOSE
    for tol in (0, 50):
        want = [fmc.expected_choice(len(f), len(h), tol)[0] for f, h in pairs]
        dst, foff, fres, tres, got = run(None, tol)
        assert got == want, (tol, [(len(f), len(h)) for f, h in pairs])
        check(pick(F, H, want), fres.cpu().tolist(), foff.cpu().tolist(), dst.cpu().numpy(), 4, fcap, ("choose", E, delta, tol))
    assert set(want) == {0, 1}
    # ... read back by the readers as they are, the delta also in place
    D = np.asarray(S, np.uint64)
    if not delta:
        back, res = hip.tensor_decompress_dbatch(dst, foff, D, E, max_total_blocks=blocks)
        assert res.cpu().tolist() == [len(t) for t in tensors] and (back.cpu().numpy()[:total] == pc.cat(tensors)).all()
    else:
        back, res = hip.tensor_decompress_delta_dbatch(dst, foff, base, D, E, max_total_blocks=blocks)
        assert res.cpu().tolist() == [len(t) for t in tensors] and (back.cpu().numpy()[:total] == pc.cat(tensors)).all()
        assert (base.cpu().numpy() == pc.cat(bases)).all()
        place = base.clone()
        _, res = hip.tensor_decompress_delta_dbatch(dst, foff, place, D, E, dst=place, dst_capacity=total, max_total_blocks=blocks)
        assert res.cpu().tolist() == [len(t) for t in tensors] and (place.cpu().numpy() == pc.cat(tensors)).all()
    # a capacity one byte short of tensor 2: it is refused (offsets are monotone, so the tensors behind it are too) between the good tensors
    # in front of it and their frames; every plane of a refused tensor is an empty content -- eight bytes, Huff0 under CHOOSE (a tie)
    k = 2
    cap = S[k + 1] - 1
    pairs = _plane_frames(checker, coded, E, cap)
    F, H = [p[0] for p in pairs], [p[1] for p in pairs]
    for codecs in (pattern, None):
        want = pattern if codecs is not None else [fmc.expected_choice(len(f), len(h), 50)[0] for f, h in pairs]
        dst, foff, fres, tres, got = run(codecs, 50, cap)
        assert tres == [len(t) for t in tensors[:k]] + [GENERIC] * (n - k) and got == want
        check(pick(F, H, want), fres.cpu().tolist(), foff.cpu().tolist(), dst.cpu().numpy(), 4, fcap, ("refused", E, delta))
        assert fres.cpu().tolist()[k * E:] == [8] * ((n - k) * E)


def test_tensor_composite_of_single_bytes(hip, checker):
    """elemBytes 1: the plain form reads the source itself and takes a null planes buffer; the delta form refuses one"""
    tensors, bases = _tensors(1)
    n, total = len(tensors), sum(len(t) for t in tensors)
    blocks = hip.planes_block_bound(total, n, 1, 0)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    pairs = _plane_frames(checker, tensors, 1)
    want = [fmc.expected_choice(len(f), len(h), 50)[0] for f, h in pairs]
    dst, foff, fres, tres, got = hip.tensor_compress_mixed_dbatch(src, pc.offsets(tensors), 1, None, None, 50, 0, max_total_blocks=blocks)      # planes None -> NULL
    sizes = [len(p[c]) for p, c in zip(pairs, want)]
    assert got.cpu().tolist() == want and fres.cpu().tolist() == sizes and foff.cpu().tolist() == fpc.packed_offsets(sizes, 0)
    out = dst.cpu().numpy()
    for i, (p, c) in enumerate(zip(pairs, want)):
        assert (out[int(foff[i]):int(foff[i]) + sizes[i]] == p[c]).all(), i
    poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(hip.frame_mixed_workspace_bound(n, blocks, 0), dtype=torch.uint8, device="cuda")
    rc = hip.lib.FSEHIP_tensor_compress_mixed_dbatch(VP(dst.data_ptr()), C.c_uint64(dst.numel()), VP(foff.data_ptr()), VP(fres.data_ptr()), VP(tres.data_ptr()),
                                                     VP(src.data_ptr()), VP(base.data_ptr()), VP(_i64(pc.offsets(tensors)).data_ptr()), SZ(n), C.c_uint(1), C.c_uint64(total),
                                                     SZ(blocks), C.c_uint(0), VP(got.data_ptr()), C.c_int(CHOOSE), C.c_uint(50), C.c_uint(0), VP(0), VP(poff.data_ptr()),
                                                     VP(ws.data_ptr()), SZ(ws.numel()), VP(torch.cuda.current_stream().cuda_stream))
    assert rc == 1, "the XOR has to be written somewhere"
    torch.cuda.synchronize()
    assert fres.cpu().tolist() == sizes and poff.cpu().tolist() == [0] * (n + 1)


# ---------------------------------------------------------------------------------------------------------------- graph
def test_choose_and_packed_reader_in_one_hip_graph(hip, checker):
    """one captured graph: CHOOSE compress at tolerance 50, then the packed reader fed with the offsets just produced.  Replayed after the
    source has changed so that frame 0's choice flips: the delta's high plane (FSE: Huff0 costs many times more) against noise (a tie: Huff0)."""
    planes = dict(fmc.update_planes())
    rng = np.random.default_rng(77)
    size = 6000
    loads = [[planes["delta_plane1"][:size], planes["delta_plane0"][:size], np.full(size, 3, np.uint8)],
             [rng.integers(0, 256, size, dtype=np.uint8), planes["delta_plane0"][size:2 * size], planes["delta_plane1"][size:2 * size]]]
    n, total, ALIGN = 3, 3 * size, 4
    promise = 3 * fmc.block_count(size, 0) + 5
    fcap = hip.frame_packed_bound(total, n, promise, ALIGN)
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff = _i64(pc.offsets(loads[0]))
    wws = torch.empty(hip.frame_mixed_workspace_bound(n, promise, 0), dtype=torch.uint8, device="cuda")
    hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize.restype = SZ
    rws = torch.empty(int(hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize(SZ(n), SZ(promise))), dtype=torch.uint8, device="cuda")
    frames, back = _filled(fcap), _filled(total)
    foff, boff = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    wres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    codecs = torch.full((n,), 7, dtype=torch.uint8, device="cuda")

    def work():
        hip.lib.FSEHIP_frame_compress_packed_mixed_dbatch.restype = C.c_int
        assert raw(hip, frames, fcap, foff, wres, src, soff, n, promise, 0, codecs, CHOOSE, 50, ALIGN, wws) == 0
        hip.frame_decompress_packed_dbatch(frames, foff, dst=back, capacity=total, max_total_blocks=promise, align_log=0, dst_offsets=boff, workspace=rws, results=rres)
    src.copy_(_dev(pc.cat(loads[1]))); work(); torch.cuda.synchronize()      # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    seen = []
    for contents in loads:
        src.copy_(_dev(pc.cat(contents)))
        frames.fill_(FILL); back.fill_(FILL); codecs.fill_(7)
        for t in (foff, boff, wres, rres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        pairs = [tuple(f[:r].copy() for r, f in (checker.frame_compress(np.ascontiguousarray(d), 0, c) for c in (0, 1))) for d in contents]
        want = [fmc.expected_choice(len(f), len(h), 50)[0] for f, h in pairs]
        seen.append(want)
        assert codecs.cpu().tolist() == want
        check([p[c] for p, c in zip(pairs, want)], wres.cpu().tolist(), foff.cpu().tolist(), frames.cpu().numpy(), ALIGN, fcap, want)
        assert rres.cpu().tolist() == [size] * n and boff.cpu().tolist() == [0, size, 2 * size, 3 * size]
        out = back.cpu().numpy()
        assert (out[:total] == pc.cat(contents)).all() and (out[total:] == FILL).all()
    assert seen[0][0] == 0 and seen[1][0] == 1, "frame 0's choice flips between the replays"


# ---------------------------------------------------------------------------------------------------------------- the pair
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_compress_tensors_with_an_auto_codec_and_with_its_codecs_again(hip, monkeypatch):
    from finitestateentropy_amd.api import AutoCodec
    gen = torch.Generator(device="cuda").manual_seed(19)
    old_np, new_np = pdc.bf16_update_pair(1 << 15)
    new2_np = pdc.bf16_update_pair(1 << 15, step=3e-5)[1]
    old_bf, new_bf, new2_bf = (torch.from_numpy(x.copy()).cuda().view(torch.bfloat16).reshape(128, 256) for x in (old_np, new_np, new2_np))
    old_f = torch.randn((700, 3), generator=gen, device="cuda") * 0.02
    new_f = old_f + torch.randn((700, 3), generator=gen, device="cuda") * 2e-5
    new2_f = old_f + torch.randn((700, 3), generator=gen, device="cuda") * 2e-5
    old_i = torch.randint(-128, 128, (4, 50), generator=gen, device="cuda", dtype=torch.int8)
    new_i = old_i.clone(); new_i[1, ::7] += 1
    old, new, new2 = [old_bf, old_f, old_i], [new_bf, new_f, new_i], [new2_bf, new2_f, new_i.clone()]
    obj = hip.compress_tensors(new, codec=AutoCodec(50), base=old)
    assert obj.delta is True and obj.codec == AutoCodec(50) and sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4]
    for g in obj.groups:
        c = g["codecs"]
        assert c.is_cuda and c.dtype == torch.uint8 and c.numel() == len(g["index"]) * g["elem_bytes"] and set(c.cpu().tolist()) <= {0, 1}
    bf = [g for g in obj.groups if g["elem_bytes"] == 2][0]
    assert bf["codecs"].cpu().tolist() == [1, 0], "the delta's low plane to the fast decoder, its high plane to the small coder"
    for a, b in zip(new, hip.decompress_tensors(obj, base=old)):
        assert a.dtype == b.dtype and a.shape == b.shape and _bits(a, b)
    plain = hip.compress_tensors(new, codec=AutoCodec(20))
    assert plain.delta is False and all("codecs" in g for g in plain.groups)
    for a, b in zip(new, hip.decompress_tensors(plain)):
        assert _bits(a, b)
    assert all("codecs" not in g for g in hip.compress_tensors(new, codec=1).groups)
    # the earlier object as `codec`: its codecs given again -- the frames of a GIVEN call with them
    again = hip.compress_tensors(new2, codec=obj, base=old)
    assert again.codec == AutoCodec(50) and again.delta is True
    for g, e in zip(again.groups, obj.groups):
        assert torch.equal(g["codecs"], e["codecs"])
        E, idx = g["elem_bytes"], g["index"]
        raw_new = torch.cat([new2[i].contiguous().reshape(-1).view(torch.uint8) for i in idx])
        raw_old = torch.cat([old[i].contiguous().reshape(-1).view(torch.uint8) for i in idx])
        offs = np.concatenate([[0], np.cumsum(g["sizes"])]).astype(np.uint64)
        dst, foff, fres, _, _ = hip.tensor_compress_mixed_dbatch(raw_new, offs, E, raw_old, e["codecs"])
        assert torch.equal(foff, g["frame_offsets"]) and torch.equal(fres, g["frame_results"]) and torch.equal(dst[:int(foff[-1])], g["frames"])
    for a, b in zip(new2, hip.decompress_tensors(again, base=old)):
        assert _bits(a, b)

    # every mismatch is raised before a launch: from here on a call into the library is a failure of the test
    def no_launch(*args):
        raise AssertionError("the library was called")
    for name in ("FSEHIP_tensor_compress_mixed_dbatch", "FSEHIP_tensor_compress_dbatch", "FSEHIP_tensor_compress_delta_dbatch"):
        monkeypatch.setattr(hip.lib, name, no_launch)
    with pytest.raises(ValueError):
        hip.compress_tensors(new2[:-1], codec=obj, base=old[:-1])                          # another count
    with pytest.raises(ValueError):
        hip.compress_tensors([new2_bf.reshape(-1)] + new2[1:], codec=obj, base=[old_bf.reshape(-1)] + old[1:])      # another shape
    with pytest.raises(ValueError):
        hip.compress_tensors([new2_bf.view(torch.float16)] + new2[1:], codec=obj, base=[old_bf.view(torch.float16)] + old[1:])      # another dtype
    with pytest.raises(ValueError):
        hip.compress_tensors(new2, codec=hip_plain_object(), base=old)                     # an object that carries no codecs


def hip_plain_object():
    from finitestateentropy_amd import api
    return api.CompressedTensors([dict(elem_bytes=2)], [torch.bfloat16], [(128, 256)], torch.device("cuda", 0), 0, 5)
