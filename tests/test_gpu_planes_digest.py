"""Tensor digests and the gate on the device (FSEHIP_tensor_digest_dbatch, FSEHIP_tensor_gate_dbatch and the Python surface around
DeltaBase(check=True)) against the numpy model of planes_digest_corpus.py, bit for bit; then the gate in front of the existing readers: the
sender's frames are made from `old`, the receiver holds a `stale` base that differs in one tensor of three, in place -- the stale tensor keeps
every byte and gets an error, the others become `new`, and with matching digests the gated call is the ungated one byte for byte.  Every output
has a mark or 0xA5 behind it that must still be there afterwards."""
import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_digest_corpus as dg
from planes_digest_corpus import CORRUPT, GENERIC, T

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, -7
M64 = (1 << 64) - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _bits64(values):
    """unsigned 64-bit values as the int64 tensor of the same bits"""
    return torch.from_numpy(np.asarray([int(v) & M64 for v in values], dtype=np.uint64).astype(np.int64)).cuda()


def _marked(n):
    return torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")


def _filled(n, shift=0, content=None):
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


# ---------------------------------------------------------------------------------------------------------------- the digest
def run_digest(hip, flat, offsets, shift=0, capacity=None):
    """-> (digests as unsigned ints, results): guard entries behind both outputs, a workspace of exactly the bound with 0xA5 behind it"""
    n = len(offsets) - 1
    cap = len(flat) if capacity is None else capacity
    src = _filled(len(flat), shift, flat)
    dig, res = _marked(n), _marked(n)
    bound = hip.tensor_digest_workspace_bound(cap, n)
    ws = torch.full((bound + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    hip.tensor_digest_dbatch(src[:max(len(flat), 1)], _i64(offsets), capacity=cap, digests=dig, results=res, workspace=ws[:max(bound, 1)])
    torch.cuda.synchronize()
    assert int(dig[n]) == MARK and int(res[n]) == MARK and (ws[bound:] == FILL).all(), "guards"
    assert (src.cpu().numpy()[:len(flat)] == flat).all() and (src[len(flat):] == FILL).all(), "the source is only read"
    return [d & M64 for d in dig.cpu().tolist()[:n]], res.cpu().tolist()[:n]


def _packed(tensors, residues, seed):
    """the tensors back to back with a filler tensor in front of each, so that tensor k starts at residues[k] mod 16: -> (units, the
    positions of the tensors among them)"""
    rng = np.random.default_rng(seed)
    units, at, where = [], 0, []
    for t, r in zip(tensors, residues):
        pad = (r - at) % 16
        units.append(rng.integers(0, 256, pad, dtype=np.uint8))
        where.append(len(units))
        units.append(t)
        at += pad + len(t)
    return units, where


SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 5, 3 * T + 1024 + 3]


@pytest.fixture(scope="module")
def sized():
    tensors = pc.random_tensors(SIZES, 41)
    return tensors, [dg.tensor_digest(t) for t in tensors]


def test_digest_against_the_model_at_every_alignment(hip, sized):
    tensors, want = sized
    assert len(set(want)) == len(want)
    seen = []
    for order, residues, shift, seed in ((range(16), [(3 + 5 * k) % 16 for k in range(16)], 1, 1), (range(15, -1, -1), [(7 * k + 2) % 16 for k in range(16)], 6, 2)):
        order = list(order)
        assert len(set(residues)) == 16, "every tensor start is off 16-byte alignment by another amount"
        units, where = _packed([tensors[k] for k in order], residues, seed)
        U = [int(x) for x in pc.offsets(units)]
        assert [U[w] % 16 for w in where] == residues
        digs, res = run_digest(hip, pc.cat(units), U, shift)
        assert res == [len(u) for u in units]
        assert [digs[w] for w in where] == [want[k] for k in order], [k for w, k in zip(where, order) if digs[w] != want[k]]
        fillers = [i for i in range(len(units)) if i not in where]
        assert [digs[i] for i in fillers] == [dg.tensor_digest(units[i]) for i in fillers]
        seen.append({k: digs[w] for w, k in zip(where, order)})
    assert seen[0] == seen[1], "another order, other offsets, the same values"


def test_digest_of_many_tiny_tensors_inside_one_tile(hip):
    rng = np.random.default_rng(42)
    tiny = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in list(range(41)) + [0, 0, 1, 40, 33, 16, 17, 15, 0, 8, 24, 32, 31, 5, 0, 0, 2, 39, 40]]
    assert len(tiny) == 60
    large = rng.integers(0, 256, 3 * T + 100, dtype=np.uint8)
    for units in (tiny + [large], [large] + tiny, tiny[:30] + [large] + tiny[30:]):
        digs, res = run_digest(hip, pc.cat(units), [int(x) for x in pc.offsets(units)], 3)
        assert res == [len(u) for u in units] and digs == [dg.tensor_digest(u) for u in units]
    digs, res = run_digest(hip, np.zeros(0, np.uint8), [0])                           # no tensors at all is legal
    assert digs == [] and res == []
    digs, res = run_digest(hip, np.zeros(0, np.uint8), [0, 0, 0])
    assert digs == [dg.tensor_digest(np.zeros(0, np.uint8))] * 2 and res == [0, 0]


def test_digest_of_tensors_whose_top_level_takes_every_path(hip):
    """the top level hashes 8 nt + 8 bytes per tensor: below 127 tiles the eight-wide loop and the single stripes, from 127 tiles (64 stripes)
    the ring of loads ahead of the chain, from 255 its refill loop -- both sides of both thresholds, a ragged tail, odd offsets, small
    neighbours; each against the model"""
    tiles = [126, 127, 201, 254, 255, 301]
    assert [(8 * nt + 8) // 16 >= 64 for nt in tiles] == [False, True, True, True, True, True]
    assert [((8 * nt + 8) // 16) // 16 - 4 >= 4 for nt in tiles[1:]] == [False, False, False, True, True]
    sizes = [37, 125 * T + 1, 5, 126 * T + 4097, 0, 200 * T + 5, 1, 253 * T + T - 1, 3, 254 * T + 16, 21, 300 * T + 1027]
    assert [-(-n // T) for n in sizes[1::2]] == tiles
    units = pc.random_tensors(sizes, 44)
    U = [int(x) for x in pc.offsets(units)]
    assert all(U[k] % 16 for k in range(1, len(units), 2)), "every large tensor starts off 16-byte alignment"
    digs, res = run_digest(hip, pc.cat(units), U, 7)
    assert res == sizes
    want = [dg.tensor_digest(u) for u in units]
    assert digs == want, [k for k in range(len(units)) if digs[k] != want[k]]


def test_digest_refuses_a_decreasing_slot_and_one_behind_the_capacity(hip):
    flat = np.random.default_rng(43).integers(0, 256, 320, dtype=np.uint8)
    offsets = [0, 100, 60, 200, 300, 370]
    digs, res = run_digest(hip, flat, offsets, 5, capacity=320)
    want, wres = dg.digest_batch(flat, offsets, 320)
    assert wres == [100, GENERIC, 140, 100, GENERIC] and res == wres and digs == want and digs[1] == digs[4] == 0


# ---------------------------------------------------------------------------------------------------------------- the gate
def run_gate(hip, F, E, got, res, want, first):
    nF, nT = len(F) - 1, len(want)
    G, R = _marked(nF + 1), _marked(nT)
    hip.tensor_gate_dbatch(_i64(F), _bits64(got), _i64(res), _bits64(want), E, frame_first=None if first is None else np.asarray(first, np.uint64), n_frames=nF,
                           gated_offsets=G, results=R)
    torch.cuda.synchronize()
    assert int(G[nF + 1]) == MARK and int(R[nT]) == MARK
    return G.cpu().tolist()[:nF + 1], R.cpu().tolist()[:nT]


def test_gate_against_the_model(hip):
    for name, F, E, got, res, want, first in dg.gate_cases():
        assert run_gate(hip, F, E, got, res, want, first) == dg.gate(F, E, got, res, want, first), name
    assert run_gate(hip, [9], 2, [], [], [], None) == ([9], [])


# ---------------------------------------------------------------------------------------------------------------- the gate in front of the readers
SEG_LOG = 10
_UPDATES = {}


def _update(E):
    """(old, new, stale) as lists of three byte arrays: bf16 (E == 2) or fp32 (E == 4) weights of T, 2 T + 5 and T - 3 elements, an update
    step on them, and `old` with one element of tensor 1 changed"""
    if E not in _UPDATES:
        counts = [T, 2 * T + 5, T - 3]
        w = np.random.default_rng(1).normal(0, 0.02, sum(counts)).astype(np.float32)
        w2 = (w + np.random.default_rng(2).normal(0, 2e-5, sum(counts))).astype(np.float32)
        old, new = (pdc.bf16_bytes(x) if E == 2 else x.view(np.uint8) for x in (w, w2))
        cuts = [E * int(c) for c in np.concatenate([[0], np.cumsum(counts)])]
        old, new = ([np.ascontiguousarray(x[a:b]) for a, b in zip(cuts, cuts[1:])] for x in (old, new))
        stale = [o.copy() for o in old]
        stale[1][150 * E + E - 1] ^= 0x01                                             # inside the window of the window case
        _UPDATES[E] = (old, new, stale)
    return _UPDATES[E]


WINDOW = (100, 300)                                                                   # elements: inside segment 0 of every plane


def _reader(hip, kind, E, op, old, new):
    """the sender's frames of `new` against `old` -> (frame offsets, seg_first or None, read(G, resident) -> results)"""
    S = pc.offsets(old)
    sizes, total, n = [len(t) for t in old], int(S[-1]), len(old)
    src, base = _dev(pc.cat(new)), _dev(pc.cat(old))
    blocks = hip.planes_block_bound(total, n, E, 0)
    if kind == "delta":
        frames, foff, fres, tres = hip.tensor_compress_delta_dbatch(src, base, S, E, 0, 0, delta_op=op)
        return foff, None, lambda G, dst: hip.tensor_decompress_delta_dbatch(frames, G, dst, S, E, dst=dst, max_total_blocks=blocks, delta_op=op)[1]
    first = hip.planes_segment_first(sizes, E, SEG_LOG)
    if kind == "sparse":
        frames, foff = hip.tensor_compress_seg_sparse_dbatch(src, S, E, SEG_LOG, 500, first, base=base, block_size_id=0, delta_op=op)[:2]
        return foff, first, lambda G, dst: hip.tensor_decompress_seg_sparse_dbatch(frames, G, S, E, SEG_LOG, first, base=dst, dst=dst, max_total_blocks=blocks,
                                                                                   delta_op=op)[1]
    frames, foff = hip.tensor_compress_seg_dbatch(src, S, E, SEG_LOG, first, base=base, block_size_id=0, delta_op=op)[:2]
    if kind == "seg":
        return foff, first, lambda G, dst: hip.tensor_decompress_seg_dbatch(frames, G, S, E, SEG_LOG, first, base=dst, dst=dst, max_total_blocks=blocks, delta_op=op)[1]
    wins = [WINDOW] * n
    D = np.concatenate([[0], np.cumsum([E * (b - a) for a, b in wins])]).astype(np.uint64)
    return foff, first, lambda G, dst: hip.tensor_decompress_window_dbatch(frames, G, S, wins, D, E, SEG_LOG, first, base=dst, dst=dst, block_size_id=0, delta_op=op)[1]


@pytest.mark.parametrize("E", (2, 4))
@pytest.mark.parametrize("kind,op", (("delta", 0), ("delta", 1), ("seg", 1), ("window", 1), ("sparse", 1)))
def test_gate_in_front_of_the_readers(hip, kind, op, E):
    old, new, stale = _update(E)
    S = [int(x) for x in pc.offsets(old)]
    n = len(old)
    foff, first, read = _reader(hip, kind, E, op, old, new)
    expected = hip.tensor_digest_dbatch(_dev(pc.cat(old)), S)[0]
    assert [d & M64 for d in expected.cpu().tolist()] == [dg.tensor_digest(t) for t in old]

    def cut(tensors):                                          # what the reader's destination holds: the tensors, or their windows
        return pc.cat(tensors) if kind != "window" else pc.cat([t[E * WINDOW[0]:E * WINDOW[1]] for t in tensors])
    ends = np.concatenate([[0], np.cumsum([len(t) if kind != "window" else E * (WINDOW[1] - WINDOW[0]) for t in old])])

    def resident(tensors):
        whole = _dev(pc.cat(tensors))
        dig, res = hip.tensor_digest_dbatch(whole, S)
        G, R = hip.tensor_gate_dbatch(foff, dig, res, expected, E, frame_first=first)
        return G, R.cpu().tolist(), _filled(len(cut(tensors)), 0, cut(tensors))

    # the receiver holds `stale`: tensor 1 keeps every byte and gets an error, the others become `new`
    G, R, dst = resident(stale)
    assert R == [len(old[0]), CORRUPT, len(old[2])]
    gated = G.cpu().tolist()
    assert all(a <= b for a, b in zip(gated, gated[1:])) and gated[-1] == int(foff[-1])
    res = read(G, dst[:len(cut(stale))])
    torch.cuda.synchronize()
    got, back = res.cpu().tolist(), dst.cpu().numpy()
    assert got[1] < 0 and [got[0], got[2]] == [int(ends[1] - ends[0]), int(ends[3] - ends[2])], got
    want = cut([new[0], stale[1], new[2]])
    assert (back[:len(want)] == want).all(), np.nonzero(back[:len(want)] != want)[0][:8]
    assert (back[len(want):] == FILL).all()
    assert not (cut(stale)[ends[1]:ends[2]] == cut(new)[ends[1]:ends[2]]).all() and not (cut(stale) == cut(old)).all()
    # matching digests: the gated offsets are the frame offsets, and the read is the ungated one byte for byte
    G, R, dst = resident(old)
    assert R == [len(t) for t in old] and torch.equal(G, foff[:G.numel()])
    plain = _filled(len(cut(old)), 0, cut(old))
    res, pres = read(G, dst[:len(cut(old))]), read(foff, plain[:len(cut(old))])
    torch.cuda.synchronize()
    assert res.cpu().tolist() == pres.cpu().tolist() == [int(b - a) for a, b in zip(ends, ends[1:])]
    assert torch.equal(dst, plain) and (dst.cpu().numpy()[:len(cut(new))] == cut(new)).all()


def test_digest_gate_and_in_place_read_in_one_hip_graph(hip):
    """one captured graph -- a single stream, a linear chain, the process's default queues -- holding the digest of the resident tensors, the
    gate and the in-place delta read; replayed over a good base, then over a base changed between the replays"""
    import ctypes as C
    E, op = 2, 1
    old, new, stale = _update(E)
    n, S = len(old), pc.offsets(old)
    total = int(S[-1])
    blocks = hip.planes_block_bound(total, n, E, 0)
    frames, foff, _, _ = hip.tensor_compress_delta_dbatch(_dev(pc.cat(new)), _dev(pc.cat(old)), S, E, 0, 0, delta_op=op)
    soff = _i64(S)
    expected = hip.tensor_digest_dbatch(_dev(pc.cat(old)), soff)[0]
    rsize = hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    rsize.restype = C.c_size_t
    rws = torch.empty(int(rsize(C.c_size_t(n * E), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    dws = torch.empty(hip.tensor_digest_workspace_bound(total, n), dtype=torch.uint8, device="cuda")
    dst, planes = _filled(total), _filled(total)
    dig, dres, gres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(4))
    G, poff = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    pres = torch.zeros(n * E, dtype=torch.int64, device="cuda")

    def work():
        hip.tensor_digest_dbatch(dst[:total], soff, capacity=total, digests=dig, results=dres, workspace=dws)
        hip.tensor_gate_dbatch(foff, dig, dres, expected, E, n_frames=n * E, gated_offsets=G, results=gres)
        hip.tensor_decompress_delta_dbatch(frames, G, dst[:total], soff, E, dst=dst[:total], dst_capacity=total, max_total_blocks=blocks, planes=planes[:total],
                                           planes_capacity=total, plane_offsets=poff, plane_results=pres, workspace=rws, results=rres, delta_op=op)
    dst[:total] = _dev(pc.cat(old)); work(); torch.cuda.synchronize()                  # one ordinary call first
    assert (dst.cpu().numpy()[:total] == pc.cat(new)).all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for held, want, verdict in ((old, new, [len(t) for t in old]), (stale, [new[0], stale[1], new[2]], [len(old[0]), CORRUPT, len(old[2])])):
        dst[:total] = _dev(pc.cat(held))
        for t in (dig, dres, gres, rres, G):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert gres.cpu().tolist() == verdict
        got = rres.cpu().tolist()
        assert [r if v >= 0 else (r < 0) for r, v in zip(got, verdict)] == [v if v >= 0 else True for v in verdict], got
        back = dst.cpu().numpy()
        assert (back[:total] == pc.cat(want)).all() and (back[total:] == FILL).all()
        assert [d & M64 for d in dig.cpu().tolist()] == [dg.tensor_digest(t) for t in held]


# ---------------------------------------------------------------------------------------------------------------- Python
def _same(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.fixture(scope="module")
def mixed():
    """old and new of mixed dtypes, and `stale`: old with tensor 2 changed"""
    gen = torch.Generator(device="cuda").manual_seed(13)
    old_np, new_np = pdc.bf16_update_pair(1 << 16)
    old = [torch.from_numpy(old_np.copy()).cuda().view(torch.bfloat16).reshape(256, 256), torch.randn((1000, 3), generator=gen, device="cuda") * 0.02,
           torch.randn((T // 4 + 3,), generator=gen, device="cuda") * 0.02, torch.arange(77, device="cuda", dtype=torch.uint8),
           torch.arange(-50, 50, device="cuda", dtype=torch.int64), torch.zeros((0, 4), device="cuda", dtype=torch.float16)]
    new = [torch.from_numpy(new_np.copy()).cuda().view(torch.bfloat16).reshape(256, 256), old[1] + 1e-5, old[2] * 1.0001, old[3] + 1, old[4] + 3, old[5].clone()]
    stale = [t.clone() for t in old]
    stale[2][T // 8] += 1.0
    return old, new, stale


def test_tensor_digests_equal_the_model(hip, mixed):
    import finitestateentropy_amd
    old, _, stale = mixed
    tensors = old + [old[0].t(), torch.ones(5, device="cuda", dtype=torch.bool), torch.ones(3, device="cuda", dtype=torch.complex64)]      # any dtype, not contiguous
    want = [dg.tensor_digest(t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()) for t in tensors]
    assert hip.tensor_digests(tensors) == want and finitestateentropy_amd.tensor_digests(tensors[::-1]) == want[::-1]
    assert hip.tensor_digests(tensors[2:3]) == want[2:3] != hip.tensor_digests(stale[2:3]), "the values do not depend on the grouping"


@pytest.mark.parametrize("segmented", (False, True))
def test_checked_delta_round_trip_and_refusal(hip, mixed, segmented):
    from finitestateentropy_amd.api import DeltaBase, SparsePlanes
    old, new, stale = mixed
    write = (lambda *a, **k: hip.compress_tensors_segmented(*a, segment_log=15, **k)) if segmented else hip.compress_tensors
    obj = write(new, codec=SparsePlanes(1), base=DeltaBase(old, "sub", check=True))
    assert obj.base_digests == hip.tensor_digests(old) and obj.delta_op == "sub" and obj.sparse_permille == 500
    back = hip.decompress_tensors(obj, DeltaBase(old, "sub"))
    assert all(_same(a, b) and a.dtype == b.dtype and a.shape == b.shape for a, b in zip(back, new))
    held = [t.clone() for t in stale]
    with pytest.raises(ValueError, match=r"tensors \[2\]"):
        hip.decompress_tensors(obj, held)
    assert all(_same(a, b) for a, b in zip(held, stale)), "every tensor passed as base is unchanged"
    two = [t.clone() for t in stale]
    two[4] = two[4] + 1
    with pytest.raises(ValueError, match=r"tensors \[2, 4\]"):
        hip.decompress_tensors(obj, two)
    # the dense codecs carry the digests too; an object written without check decodes over the stale base without complaint, as today
    dense = write(new, codec=0, base=DeltaBase(old, "xor", check=True))
    assert dense.base_digests == obj.base_digests and all(_same(a, b) for a, b in zip(hip.decompress_tensors(dense, old), new))
    with pytest.raises(ValueError, match=r"tensors \[2\]"):
        hip.decompress_tensors(dense, stale)
    plain = write(new, codec=SparsePlanes(1), base=DeltaBase(old, "sub"))
    assert plain.base_digests is None and "base_digests" not in vars(plain)
    wrong = hip.decompress_tensors(plain, stale)
    assert not _same(wrong[2], new[2]) and all(_same(a, b) for k, (a, b) in enumerate(zip(wrong, new)) if k != 2)


def test_windows_and_patches_do_not_check_and_patches_carry_the_digests(hip, mixed):
    from finitestateentropy_amd.api import DeltaBase
    old, new, stale = mixed
    obj = hip.compress_tensors_segmented(new, segment_log=15, base=DeltaBase(old, "sub", check=True))
    wins = [None, None, (0, 16), None, None, None]
    got = hip.decompress_tensor_windows(obj, wins, stale)                              # (the changed element lies outside the window)
    assert _same(got[2], new[2].reshape(-1)[:16])
    patched = hip.patch_tensor_windows(obj, new, [None] * len(new), old)
    assert patched.base_digests == obj.base_digests and vars(patched)["base_digests"] is not obj.base_digests
    assert all(_same(a, b) for a, b in zip(hip.decompress_tensors(patched, old), new))
