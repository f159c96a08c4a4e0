"""Byte planes of tensors on the device (FSEHIP_planes_split_dbatch / _merge_dbatch, FSEHIP_tensor_compress_dbatch / _decompress_dbatch and the
compress_tensors pair) against the numpy model of planes_corpus.py -- plane p of a tensor is raw[p::E] -- and the CPU oracle's frames of those
planes, laid out as frame_packed_corpus's model of the packed writer places them; never against the library's own calls.  Block-size id 0 (1 KB
blocks) wherever frames are involved.  Every destination is filled with 0xA5 and has a tail behind it: whatever the contract does not give to
the call must still be 0xA5 afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_packed_corpus as fpc
import planes_corpus as pc
from planes_corpus import CORRUPT, GENERIC, TILE, TOO_SMALL

pytestmark = pytest.mark.gpu

FILL, TAIL = 0xA5, 64
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _filled(n, shift=0):
    """n + TAIL bytes of FILL starting `shift` bytes behind an allocation's (256-byte aligned) start"""
    return torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]


def _batches(E):
    """the two batches of the issue: the size list (random bytes), and 3,000 tensors of 0..40 bytes -- many tensors per tile"""
    if E not in _CACHE:
        rng = np.random.default_rng(100 + E)
        _CACHE[E] = (pc.random_tensors(pc.split_sizes(E), 7 + E), pc.random_tensors(rng.integers(0, 41, 3000), 70 + E))
    return _CACHE[E]


def run_split(hip, tensors, E, capacity=None, shift=(0, 0)):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    src = _filled(total, shift[0])
    src[:total] = _dev(pc.cat(tensors))
    planes = _filled(total, shift[1])
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_split_dbatch(src[:total], S, E, capacity=capacity, planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, E, capacity=None):
    out, poff, res = got
    want, written, P, wres = pc.split_model(tensors, E, capacity)
    if E == 1:
        written[:] = False                                   # offsets and results only: no byte of the planes buffer is the call's
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_against_the_model(hip, E):
    sized, many = _batches(E)
    assert [len(t) for t in sized][:3] == [1, E + 1, 15] and max(len(t) for t in sized) == 3 * TILE + 5
    check_split(run_split(hip, sized, E), sized, E)
    check_split(run_split(hip, sized, E, shift=(5, 3)), sized, E)            # buffers that start off every boundary
    assert len(many) == 3000 and int(pc.offsets(many)[-1]) > TILE
    check_split(run_split(hip, many, E), many, E)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_with_a_short_capacity(hip, E):
    sized, many = _batches(E)
    S = [int(x) for x in pc.offsets(sized)]
    k = 11                                                   # the tensor of one tile less a byte
    assert len(sized[k]) == TILE - 1
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):  # inside a tensor, at a tensor's end, one short of it, at an early end, nothing
        got = run_split(hip, sized, E, capacity=cap)
        check_split(got, sized, E, cap)
        first = next(i for i in range(len(sized)) if S[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (len(sized) - first) and got[1][first * E:] == [S[first]] * (len(got[1]) - first * E)
    Sm = [int(x) for x in pc.offsets(many)]
    cap = Sm[1500] + 1
    check_split(run_split(hip, many, E, capacity=cap), many, E, cap)


# ---------------------------------------------------------------------------------------------------------------- 3
def run_merge(hip, E, planes_buf, poff, psizes, D, capacity=None, room=None, shift=(0, 0)):
    n = len(D) - 1
    room = int(D[-1]) if room is None else room
    planes = _filled(len(planes_buf), shift[0])
    planes[:len(planes_buf)] = _dev(planes_buf)
    dst = _filled(room, shift[1])
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_merge_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), np.asarray(D, np.uint64), E, dst=dst,
                            capacity=room if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == -7
    return dst.cpu().numpy(), res.cpu().tolist()[:n]


def check_merge(got, tensors, E, psizes, D, capacity):
    out, res = got
    want = [pc.merge_verdict(psizes[i * E:(i + 1) * E], int(D[i + 1]), int(D[i]), E, capacity) for i in range(len(tensors))]
    assert res == want
    written = np.zeros(len(out), bool)
    for i, raw in enumerate(tensors):
        if want[i] >= 0:
            assert want[i] == len(raw)
            assert (out[int(D[i]):int(D[i]) + len(raw)] == raw).all(), i
            written[int(D[i]):int(D[i]) + len(raw)] = True
    assert (out[~written] == FILL).all(), ("bytes outside the good tensors", np.nonzero((out != FILL) & ~written)[0][:8])
    return want


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_against_the_model(hip, E):
    for tensors, shift in ((_batches(E)[0], (0, 0)), (_batches(E)[0], (3, 5)), (_batches(E)[1], (0, 0))):
        buf, _, P, _ = pc.split_model(tensors, E)
        psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
        D = [int(x) for x in pc.offsets(tensors)]
        want = check_merge(run_merge(hip, E, buf, P[:-1], psizes, D, shift=shift), tensors, E, psizes, D, D[-1])
        assert want == [len(t) for t in tensors]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_refusals(hip, E):
    tensors = _batches(E)[0]
    n = len(tensors)
    buf, _, P, _ = pc.split_model(tensors, E)
    psizes = [pc.plane_size(len(t), p, E) for t in tensors for p in range(E)]
    short, wrong, failed, behind = 9, 10, 12, n - 1             # tensors of 1024 E - 1, 1024 E + 1, T and 3 T + 5 bytes
    slots = [len(t) + (i % 3) for i, t in enumerate(tensors)]  # slots with some room to spare ...
    slots[short] = len(tensors[short]) - 1                     # ... and one a byte short
    D = [0]
    for s in slots:
        D.append(D[-1] + s)
    if E > 1:
        psizes[wrong * E] -= 1; psizes[wrong * E + 1] += 1     # the same total, not the planes of one tensor
    else:
        wrong = None
    if E >= 4:
        psizes[failed * E + 1], psizes[failed * E + 3], first = -3, -4, -3
    elif E == 2:
        psizes[failed * E], psizes[failed * E + 1], first = -3, -4, -3
    else:
        psizes[failed * E], first = -3, -3
    cap = D[n] - 1                                             # the last slot ends behind the capacity
    want = check_merge(run_merge(hip, E, buf, P[:-1], psizes, D, capacity=cap, room=D[n]), tensors, E, psizes, D, cap)
    assert want[short] == TOO_SMALL and want[failed] == first and want[behind] == GENERIC and (wrong is None or want[wrong] == CORRUPT)
    assert sum(1 for w in want if w < 0) == (4 if wrong is not None else 3)


# ---------------------------------------------------------------------------------------------------------------- 4, 5
def _tensors_of_kinds(oracle, E, seed=0):
    """tensors whose planes are, in turn, compressible (a skewed source), incompressible (random bytes: raw blocks) and constant (RLE blocks);
    plane lengths cross and miss the 1 KB block size; one tensor's size is no multiple of E, one is empty"""
    rng = np.random.default_rng(40 + E + seed)
    tensors = []
    for i, m in enumerate((3000, 1024, 5, 0, 2500, 1025)):
        raw = np.zeros(m * E + (E - 1 if i == 4 else 0), np.uint8)
        for p in range(E):
            k = len(raw[p::E])
            kind = (i + p) % 3
            raw[p::E] = (oracle.probagen_batch(20, 1, max(k, 1), 1 + seed + 10 * i + p)[0][:k] if kind == 0 else
                         rng.integers(0, 256, k, dtype=np.uint8) if kind == 1 else np.full(k, 17 + i + p + seed, np.uint8))
        tensors.append(raw)
    return tensors


def _oracle_frames(oracle, tensors, E, codec):
    out = []
    for raw in tensors:
        for pl in pc.planes_of(raw, E):
            r, f = oracle.frame_compress(np.ascontiguousarray(pl), 0, codec)
            out.append(f[:r].copy())
    return out


def _corpus(oracle, E, codec):
    key = ("kinds", E, codec)
    if key not in _CACHE:
        tensors = _tensors_of_kinds(oracle, E)
        _CACHE[key] = (tensors, _oracle_frames(oracle, tensors, E, codec))
    return _CACHE[key]


def run_compress(hip, tensors, E, codec, align_log, capacity=None):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, align_log)
    dst = _filled(fcap)
    src = _filled(total)
    src[:total] = _dev(pc.cat(tensors))
    _, foff, fres, tres = hip.tensor_compress_dbatch(src[:total], S, E, 0, codec, capacity=capacity, dst=dst, dst_capacity=fcap, max_total_blocks=blocks,
                                                     align_log=align_log)
    torch.cuda.synchronize()
    return dst, foff, fres, tres, fcap


def check_frames(want, dst, foff, fres, align_log, fcap, what):
    sizes = [len(w) for w in want]
    off, res, out = foff.cpu().tolist(), fres.cpu().tolist(), dst.cpu().numpy()
    assert off == fpc.packed_offsets(sizes, align_log, fcap), what
    assert res == fpc.packed_results(sizes, align_log, fcap) == sizes, what
    written = np.zeros(len(out), bool)
    for i, w in enumerate(want):
        assert (out[off[i]:off[i] + res[i]] == w).all(), (what, i)
        written[off[i]:off[i] + res[i]] = True
    assert (out[~written] == FILL).all(), (what, "bytes outside the frames", np.nonzero((out != FILL) & ~written)[0][:8])


@pytest.mark.parametrize("align_log", [0, 8])
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_compress_gives_the_oracles_frame_of_every_plane(hip, checker, E, codec, align_log):
    tensors, want = _corpus(checker, E, codec)
    kinds = {int(f[5]) >> 6 for f in want if len(f) > 8}
    assert kinds == {0, 1, 2}, "compressed, raw and RLE first blocks"
    dst, foff, fres, tres, fcap = run_compress(hip, tensors, E, codec, align_log)
    check_frames(want, dst, foff, fres, align_log, fcap, (E, codec, align_log))
    assert tres.cpu().tolist() == [len(t) for t in tensors]


def test_tensor_compress_of_a_refused_tensor(hip, checker):
    E, codec = 4, 0
    tensors, want = _corpus(checker, E, codec)
    S = [int(x) for x in pc.offsets(tensors)]
    k = 4
    empty = checker.frame_compress(np.zeros(0, np.uint8), 0, codec)
    empty = empty[1][:empty[0]].copy()
    assert len(empty) == 8
    dst, foff, fres, tres, fcap = run_compress(hip, tensors, E, codec, 0, capacity=S[k + 1] - 1)
    check_frames(want[:k * E] + [empty] * ((len(tensors) - k) * E), dst, foff, fres, 0, fcap, "refused")
    assert tres.cpu().tolist() == [len(t) for t in tensors[:k]] + [GENERIC] * (len(tensors) - k)


def run_decompress(hip, frames, foff, tensors, E, blocks):
    D = pc.offsets(tensors)
    total = int(D[-1])
    back = _filled(total)
    res = torch.full((len(tensors),), -7, dtype=torch.int64, device="cuda")
    hip.tensor_decompress_dbatch(frames, foff, D, E, dst=back, dst_capacity=total, max_total_blocks=blocks, results=res)
    torch.cuda.synchronize()
    return back.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("align_log", [0, 8])
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("E", pc.ELEMS)
def test_tensor_decompress_round_trip_and_a_damaged_frame(hip, checker, E, codec, align_log):
    tensors, want = _corpus(checker, E, codec)
    n, D = len(tensors), [int(x) for x in pc.offsets(tensors)]
    blocks = hip.planes_block_bound(D[-1], n, E, 0)
    dst, foff, fres, _, fcap = run_compress(hip, tensors, E, codec, align_log)
    check_frames(want, dst, foff, fres, align_log, fcap, "the frames of test 4")
    back, res = run_decompress(hip, dst, foff, tensors, E, blocks)
    assert res == [len(t) for t in tensors]
    assert (back[:D[-1]] == pc.cat(tensors)).all() and (back[D[-1]:] == FILL).all()
    # one payload byte of one plane's frame flipped: that tensor gets what the oracle's reader says of that frame, and is not written
    victim, plane = 0, (E - 1 if E > 1 else 0)
    f = victim * E + plane
    at = 5 + 3 + 40                                            # behind the frame's and the first (full, 1 KB) block's header
    assert len(want[f]) > at + 8 and want[f][5] & 0x20
    bad = want[f].copy()
    bad[at] ^= 0x55
    r, _ = checker.frame_decompress(bad, len(tensors[victim][plane::E]))
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    dst[int(foff[f]) + at] ^= 0x55
    back, res = run_decompress(hip, dst, foff, tensors, E, blocks)
    assert res == [r - (1 << 64)] + [len(t) for t in tensors[1:]]
    assert (back[:D[1]] == FILL).all() and (back[D[1]:D[-1]] == pc.cat(tensors[1:])).all() and (back[D[-1]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding tensor_compress_dbatch and then tensor_decompress_dbatch fed with the
    offsets the writer has just produced; replayed twice over other contents of the same sizes"""
    E, codec, ALIGN = 2, 0, 4
    first = _tensors_of_kinds(checker, E)
    n, S = len(first), pc.offsets(first)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, n * E, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    wws = torch.empty(int(wsize(C.c_size_t(n * E), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(rsize(C.c_size_t(n * E), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff = _i64(S)
    frames, back, planes, planes2 = _filled(fcap), _filled(total), _filled(total), _filled(total)
    foff, poff, poff2 = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    fres, pres = (torch.zeros(n * E, dtype=torch.int64, device="cuda") for _ in range(2))
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_dbatch(src, soff, E, 0, codec, dst=frames, dst_capacity=fcap, max_total_blocks=blocks, align_log=ALIGN, frame_offsets=foff,
                                   frame_results=fres, tensor_results=tres, planes=planes, plane_offsets=poff, workspace=wws)
        hip.tensor_decompress_dbatch(frames, foff, soff, E, dst=back, dst_capacity=total, max_total_blocks=blocks, planes=planes2, planes_capacity=total,
                                     plane_offsets=poff2, plane_results=pres, workspace=rws, results=rres)
    src.copy_(_dev(pc.cat(first))); work(); torch.cuda.synchronize()      # one ordinary call first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for trial in (1, 2):
        tensors = _tensors_of_kinds(checker, E, seed=trial)
        assert [len(t) for t in tensors] == [len(t) for t in first] and not (pc.cat(tensors) == pc.cat(first)).all()
        src.copy_(_dev(pc.cat(tensors)))
        for t in (frames, back):
            t.fill_(FILL)
        for t in (foff, fres, tres, rres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        check_frames(_oracle_frames(checker, tensors, E, codec), frames, foff, fres, ALIGN, fcap, trial)
        assert tres.cpu().tolist() == rres.cpu().tolist() == [len(t) for t in tensors]
        out = back.cpu().numpy()
        assert (out[:total] == pc.cat(tensors)).all() and (out[total:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_compress_tensors_and_back(hip):
    gen = torch.Generator(device="cuda").manual_seed(5)
    bits = torch.randint(-32768, 32768, (3, 5, 7), generator=gen, device="cuda", dtype=torch.int16)
    bits[0, 0, :4] = torch.tensor([0x7FC1 - 0x10000 + 0x8000, 0x7F81, -0x8000, 0x0001], dtype=torch.int16)   # NaN payloads, -0.0, a denormal
    bf = bits.view(torch.bfloat16)
    assert bool(torch.isnan(bf).any())
    half = torch.randn((6, 9), generator=gen, device="cuda").to(torch.float16).t()
    assert not half.is_contiguous()
    tensors = [bf, half, torch.randn((1000, 3), generator=gen, device="cuda"), torch.randn((17,), generator=gen, device="cuda", dtype=torch.float64),
               torch.randint(0, 256, (4, 50), generator=gen, device="cuda", dtype=torch.uint8), torch.zeros((0, 3), device="cuda", dtype=torch.float32)]
    obj = hip.compress_tensors(tensors, codec=0, block_size_id=0)
    assert sorted(g["elem_bytes"] for g in obj.groups) == [1, 2, 4, 8] and obj.nbytes > 0
    back = hip.decompress_tensors(obj)
    assert len(back) == len(tensors)
    for a, b in zip(tensors, back):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device
        assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    with pytest.raises(TypeError):
        hip.compress_tensors([torch.zeros(4, dtype=torch.complex128, device="cuda")])


# ---------------------------------------------------------------------------------------------------------------- beyond 2^31
def test_one_tensor_beyond_two_gib(hip):
    """positions past 2^31 (and 2^32 once they count elements times E): one tensor of 2 GiB + one tile + 6 bytes, checked on the device"""
    E = 4
    n = (1 << 31) + TILE + 6
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    src[:n - 6].view(torch.int64).random_()                  # (n is no multiple of 8: the last bytes get values of their own)
    src[n - 8:] = torch.arange(8, dtype=torch.uint8, device="cuda")
    planes = _filled(n)
    S = np.array([0, n], np.uint64)
    _, poff, res = hip.planes_split_dbatch(src, S, E, planes=planes)
    P = [0] + [sum(pc.plane_size(n, q, E) for q in range(p + 1)) for p in range(E)]
    assert poff.cpu().tolist() == P and res.cpu().tolist() == [n]
    for p in range(E):
        assert torch.equal(planes[P[p]:P[p + 1]], src[p::E]), p
    assert bool((planes[n:] == FILL).all())
    back = _filled(n)
    _, res = hip.planes_merge_dbatch(planes[:n], poff[:E], _i64([pc.plane_size(n, p, E) for p in range(E)]), S, E, dst=back, capacity=n)
    assert res.cpu().tolist() == [n] and torch.equal(back[:n], src) and bool((back[n:] == FILL).all())


def test_the_pair_promises_no_more_blocks_than_the_planes_can_have(hip, monkeypatch):
    """compress_tensors / decompress_tensors at the default block size (32 KB blocks): the reader's promise -- it sizes the reader's workspace and
    launches -- is planes_block_bound of the tensors, not the (F - 8) / 2 blocks per frame a reader of unknown frames has to assume; and the
    mirror's own default is the exact block count of the frames"""
    gen = torch.Generator(device="cuda").manual_seed(9)
    tensors = [(torch.randn(300001, generator=gen, device="cuda") * 0.02).to(torch.bfloat16), torch.randn((100, 1000), generator=gen, device="cuda"),
               (torch.randn(70000, generator=gen, device="cuda") * 0.02).to(torch.bfloat16)]
    obj = hip.compress_tensors(tensors)
    assert obj.block_size_id == 5 and [g["elem_bytes"] for g in obj.groups] == [2, 4]
    seen = []
    real = hip.lib.FSEHIP_tensor_decompress_dbatch
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t

    def spy(*args):
        seen.append(dict(n=args[6].value, E=args[7].value, blocks=args[8].value, ws=args[14].value))
        return real(*args)
    monkeypatch.setattr(hip.lib, "FSEHIP_tensor_decompress_dbatch", spy)
    back = hip.decompress_tensors(obj)
    for a, b in zip(tensors, back):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    assert back[0].data_ptr() != back[2].data_ptr() and back[0].untyped_storage().nbytes() == tensors[0].numel() * 2, "every tensor owns its memory"
    assert len(seen) == 2
    for s, g in zip(seen, obj.groups):
        bound = hip.planes_block_bound(sum(g["sizes"]), len(g["sizes"]), g["elem_bytes"], 5)
        assert (s["n"], s["E"]) == (len(g["sizes"]), g["elem_bytes"])
        assert s["blocks"] == bound == -(-sum(g["sizes"]) // 32768) + s["n"] * s["E"]
        assert s["ws"] == int(rsize(C.c_size_t(s["n"] * s["E"]), C.c_size_t(bound)))
    # the mirror without a promise: the exact block count of the frames, from a sizing query
    del seen[:]
    g = obj.groups[0]
    E, sizes = g["elem_bytes"], g["sizes"]
    _, res = hip.tensor_decompress_dbatch(g["frames"], g["frame_offsets"], np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), E)
    assert res.cpu().tolist() == sizes
    assert seen[0]["blocks"] == sum(-(-pc.plane_size(n, p, E) // 32768) for n in sizes for p in range(E))
