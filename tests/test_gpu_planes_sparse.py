"""Sparse planes on the device (FSEHIP_sparse_pack_dbatch, FSEHIP_sparse_expand_dbatch, the four *_sparse_dbatch composites and the Python
surface around SparsePlanes) against the numpy model of planes_sparse_corpus.py and the CPU oracle's frames of the model's contents, byte for
byte; never against the library's own calls, except where the point is that a threshold under which nothing qualifies gives the existing
composites' frames bit for bit.  Block-size id 0 wherever frames are involved, except for the recorded size table.  Every destination is
filled with 0xA5 and has a tail behind it: whatever the contract does not give to the call must still be 0xA5 afterwards, and in the
in-place form whatever the call does not own must still be the base."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mixed_corpus as fmc
import frame_packed_corpus as fpc
import planes_corpus as pc
import planes_delta_corpus as pdc
import planes_seg_corpus as pseg
import planes_sparse_corpus as sp
import planes_sub_corpus as psc
from planes_corpus import CORRUPT, GENERIC, TILE

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, -7
SHIFTS = ((0, 0), (1, 3), (8, 15), (5, 2))                  # two buffers, each off 16-byte alignment by an amount of its own
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _marked(n):
    return torch.full((n + 1,), MARK, dtype=torch.int64, device="cuda")


def _filled(n, shift=0, content=None):
    """n + TAIL bytes of FILL starting `shift` bytes behind an allocation's (256-byte aligned) start, the first bytes set to `content`"""
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _units():
    """the unit list of the issue: the sizes around a mask byte, a 16-byte piece, a lane's 64 bytes and the tile, each sparse; dozens of tiny
    units inside one tile -- empty, all zero, sparse, dense -- next to a dense and a sparse unit of several tiles; non-zeros in the last,
    partial mask byte only; and a non-zero on the first and on the last byte of every tile of the flat axis"""
    if "units" not in _CACHE:
        rng = np.random.default_rng(31)
        sizes = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
        units = [sp.with_density(n, n // 16 if n > 40 else min(n, 1), 200 + n % 97) for n in sizes]
        for k in range(60):                                  # tiny units, 1.5 KB in all: many unit boundaries in one tile
            n = int(rng.integers(0, 50))
            units.append([np.zeros(n, np.uint8), sp.with_density(n, n // 5, k), rng.integers(1, 256, n, dtype=np.uint8)][k % 3])
        units.append(rng.integers(1, 256, 2 * TILE + 100, dtype=np.uint8))              # dense, copied tile by tile
        units.append(sp.with_density(2 * TILE + 77, TILE // 3, 5))                      # sparse over several tiles, values crossing the tiles
        tail = np.zeros(4099, np.uint8)
        tail[4096:] = (9, 8, 7)                                                        # non-zeros in the last, partial mask byte only
        units.append(tail)
        units.append(sp.with_density(TILE // 2 + 3, 0, 6))                              # all zero: a mask alone
        flat = pc.cat(units)
        for k in range(TILE, len(flat), TILE):
            flat[k - 1], flat[k] = 0x81, 0x7E
        units = sp.cut(flat, [int(x) for x in pc.offsets(units)])
        _CACHE["units"] = [np.ascontiguousarray(u) for u in units]
    return _CACHE["units"]


# ---------------------------------------------------------------------------------------------------------------- pack
def run_pack(hip, units, permille, shift=(0, 0), capacity=None):
    n, U = len(units), pc.offsets(units)
    total = int(U[-1])
    src, contents = _filled(total, shift[0], pc.cat(units)), _filled(total, shift[1])
    coff = _marked(n + 1)
    hip.sparse_pack_dbatch(src[:max(total, 1)], U, permille, capacity=total if capacity is None else capacity, contents=contents, content_offsets=coff)
    torch.cuda.synchronize()
    assert int(coff[n + 1]) == MARK
    assert (src.cpu().numpy()[:total] == pc.cat(units)).all(), "the units are only read"
    return contents.cpu().numpy(), coff.cpu().tolist()[:n + 1]


def check_pack(got, units, permille, capacity=None):
    out, coff = got
    U = [int(x) for x in pc.offsets(units)]
    seen = [u if capacity is None or U[i + 1] <= capacity else u[:0] for i, u in enumerate(units)]     # a unit behind the capacity: an empty content
    want, woff = sp.pack_model(seen, permille)
    assert coff == woff
    flat = pc.cat(want)
    assert (out[:len(flat)] == flat).all(), np.nonzero(out[:len(flat)] != flat)[0][:8]
    assert (out[len(flat):] == FILL).all(), ("bytes behind the contents", np.nonzero(out[len(flat):] != FILL)[0][:8] + len(flat))
    return want


def test_pack_against_the_model(hip):
    units = _units()
    sizes = [len(u) for u in units]
    assert sizes[:11] == [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65] and {TILE - 1, TILE, TILE + 1, 3 * TILE + 5} <= set(sizes)
    for permille in (0, 500, 1000):
        for shift in SHIFTS:
            want = check_pack(run_pack(hip, units, permille, shift), units, permille)
        forms = [len(c) < len(u) for c, u in zip(want, units)]
        assert any(forms) and not all(forms), "both forms in one call"
    assert sum(len(c) < len(u) for c, u in zip(sp.pack_model(units, 0)[0], units)) < sum(len(c) < len(u) for c, u in zip(sp.pack_model(units, 500)[0], units))


def test_pack_a_threshold_that_flips_exactly_one_unit_of_two(hip):
    a, b = sp.with_density(4000, 1000, 1), sp.with_density(4000, 1001, 2)
    p = sp.flip_permille(4000, 1000, 4000, 1001)
    assert p == 250
    for units in ([a, b], [b, a]):
        want = check_pack(run_pack(hip, units, p, SHIFTS[1]), units, p)
        assert sorted(len(c) for c in want) == [500 + 1000, 4000]
        assert all(len(c) == 4000 for c in check_pack(run_pack(hip, units, p - 1), units, p - 1))
        assert all(len(c) < 4000 for c in check_pack(run_pack(hip, units, p + 1), units, p + 1))
    # the second inequality: 64 bytes with 55 and with 56 non-zeros
    units = [sp.with_density(64, 55, 3), sp.with_density(64, 56, 4)]
    assert [len(c) for c in check_pack(run_pack(hip, units, 1000), units, 1000)] == [63, 64]


def test_pack_with_a_short_capacity(hip):
    units = _units()
    U = [int(x) for x in pc.offsets(units)]
    k = next(i for i, u in enumerate(units) if len(u) == TILE)
    for cap in (U[k] + 100, U[k + 1], U[k + 1] - 1, U[3], 0):
        out, coff = run_pack(hip, units, 500, SHIFTS[2], capacity=cap)
        check_pack((out, coff), units, 500, cap)
        first = next(i for i in range(len(units)) if U[i + 1] > cap)
        assert coff[first:] == [coff[first]] * (len(coff) - first), "units behind the capacity are empty contents"


# ---------------------------------------------------------------------------------------------------------------- expand
def run_expand(hip, contents, results, sizes, shift=(0, 0), in_units=None):
    """contents: the arrays laid back to back; results: their sizes, or a (negative) error; sizes: the dense layout"""
    n = len(sizes)
    coff = [int(x) for x in pc.offsets(contents)]
    U = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(U[-1])
    cbuf = _filled(coff[-1], shift[0], pc.cat(contents))
    units = _filled(total, shift[1], in_units)
    res = _marked(n)
    hip.sparse_expand_dbatch(cbuf[:max(coff[-1], 1)], _i64(coff), _i64(results), U, units=units, capacity=total, contents_capacity=coff[-1], results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == MARK
    assert (cbuf.cpu().numpy()[:coff[-1]] == pc.cat(contents)).all(), "the contents are only read"
    return units.cpu().numpy(), res.cpu().tolist()[:n]


def test_expand_against_the_model(hip):
    units = _units()
    sizes = [len(u) for u in units]
    U = [int(x) for x in pc.offsets(units)]
    for permille in (0, 500, 1000):
        contents, _ = sp.pack_model(units, permille)
        for shift in SHIFTS:
            out, res = run_expand(hip, contents, [len(c) for c in contents], sizes, shift)
            assert res == sizes
            assert (out[:U[-1]] == pc.cat(units)).all(), np.nonzero(out[:U[-1]] != pc.cat(units))[0][:8]
            assert (out[U[-1]:] == FILL).all()


def test_expand_refuses_what_the_reader_rule_refuses_and_writes_nothing_of_it(hip):
    victim = sp.with_density(77, 20, 9)
    victim[76] = 0
    big = sp.with_density(2 * TILE + 13, TILE // 4, 10)                                 # the same refusals over several tiles
    big[-1] = 0
    cases = sp.damaged_contents(victim) + sp.damaged_contents(big)
    good = [sp.with_density(500, 30, 70 + k) for k in range(len(cases) + 3)]
    units, contents, results, want = [], [], [], []
    for k, g in enumerate(good):                                                       # good, damaged, good, damaged, ..
        units.append(g); contents.append(sp.pack_unit(g, 1000)); results.append(len(contents[-1])); want.append(len(g))
        if k < len(cases):
            name, c, n = cases[k]
            units.append(np.zeros(n, np.uint8)); contents.append(c); results.append(len(c)); want.append(CORRUPT)
    # the frame reader's errors pass through, whatever lies in the content's slot
    for err in (-3, GENERIC):
        units.append(np.zeros(300, np.uint8)); contents.append(sp.pack_unit(good[0], 1000)); results.append(err); want.append(err)
    # a result larger than the content's slot: it does not lie inside the contents buffer
    units.append(np.zeros(40, np.uint8)); contents.append(np.ones(40, np.uint8)); results.append(41); want.append(CORRUPT)
    sizes = [len(u) for u in units]
    U = [int(x) for x in pc.offsets(units)]
    for shift in SHIFTS[:2]:
        out, res = run_expand(hip, contents, results, sizes, shift)
        assert res == want
        for i, u in enumerate(units):
            assert (out[U[i]:U[i + 1]] == (u if want[i] >= 0 else FILL)).all(), (i, "a unit that fails is not written")
        assert (out[U[-1]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- the composites
def _pairs(E):
    """(tensors, bases): an update that moves one element in eight a little -- sparse high planes for XOR and SUB -- over two segments and a bit
    of 1 << 11; nothing; noise against noise (dense planes) of exactly one segment of 1 << 10 per plane; an unchanged tensor of a size that is
    no multiple of E (all-zero planes); a short tensor"""
    if ("pairs", E) not in _CACHE:
        rng = np.random.default_rng(90 + E)
        n0 = E * (2 * 2048 + 100)
        base = rng.integers(0, 256, n0, dtype=np.uint8)
        wide = np.dtype("<u%d" % E) if E > 1 else np.uint8
        new = (base.view(wide) + (rng.integers(1, 4, n0 // E) * (rng.integers(0, 8, n0 // E) == 0)).astype(wide)).view(np.uint8)
        same = rng.integers(0, 256, E * 1500 + E - 1, dtype=np.uint8)
        tensors = [new, np.zeros(0, np.uint8), rng.integers(0, 256, E * 1024, dtype=np.uint8), same, rng.integers(0, 256, 3, dtype=np.uint8)]
        bases = [base, np.zeros(0, np.uint8), rng.integers(0, 256, E * 1024, dtype=np.uint8), same.copy(), rng.integers(0, 256, 3, dtype=np.uint8)]
        _CACHE[("pairs", E)] = (tensors, bases)
    return _CACHE[("pairs", E)]


def _data(E, form):
    tensors, bases = _pairs(E)
    return tensors if form == "plain" else psc.delta_all(tensors, bases, E, psc.SUB if form == "sub" else psc.XOR)


def _units_of(data, E, seg_log):
    if seg_log is None:
        return [np.ascontiguousarray(pl) for t in data for pl in pc.planes_of(t, E)]
    return [np.ascontiguousarray(pl[a:a + (1 << seg_log)]) for t in data for pl in pc.planes_of(t, E) for a in (range(0, len(pl), 1 << seg_log) if len(pl) else [0])]


def _frames(oracle, E, form, seg_log, permille, codec):
    """the oracle's frame of the model's content of every unit"""
    key = ("frames", E, form, seg_log, permille, codec)
    if key not in _CACHE:
        out = []
        for u in _units_of(_data(E, form), E, seg_log):
            r, f = oracle.frame_compress(sp.pack_unit(u, permille), 0, codec)
            out.append(f[:r].copy())
        _CACHE[key] = out
    return _CACHE[key]


def run_compress(hip, tensors, bases, E, op, seg_log, permille, align_log, codec=0, codecs=None, shift=(0, 0), capacity=None):
    n, S = len(tensors), pc.offsets(tensors)
    total = int(S[-1])
    sizes = [len(t) for t in tensors]
    nf = pseg.seg_first(sizes, E, seg_log)[-1] if seg_log is not None else n * E
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, nf, blocks, align_log)
    dst = _filled(fcap)
    src = _filled(total, shift[0], pc.cat(tensors))
    base = None if bases is None else _filled(total, shift[1], pc.cat(bases))[:total]
    contents = _filled(total, shift[1] + 1)
    kw = dict(base=base, codec=codec, codecs=codecs, block_size_id=0, dst=dst, dst_capacity=fcap, max_total_blocks=blocks, align_log=align_log, contents=contents,
              delta_op=op, capacity=capacity)
    if seg_log is None:
        _, foff, fres, tres, chosen = hip.tensor_compress_sparse_dbatch(src[:total], S, E, permille, **kw)
    else:
        _, foff, fres, tres, chosen = hip.tensor_compress_seg_sparse_dbatch(src[:total], S, E, seg_log, permille, **kw)
    torch.cuda.synchronize()
    assert foff.numel() == nf + 1 and fres.numel() == nf
    assert (contents.cpu().numpy()[total:] == FILL).all(), "the contents are at most the tensors' bytes"
    return dst, foff, fres, tres, chosen, fcap


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


def run_decompress(hip, frames, foff, tensors, bases, E, op, seg_log, in_place=False, shift=(0, 0)):
    D = pc.offsets(tensors)
    total = int(D[-1])
    base = None if bases is None else _filled(total, shift[0], pc.cat(bases))
    back = base if in_place else _filled(total, shift[1])
    res = _marked(len(tensors))
    kw = dict(base=base, dst=back, dst_capacity=total, max_total_blocks=hip.planes_block_bound(total, len(tensors), E, 0), results=res, delta_op=op)
    if seg_log is None:
        hip.tensor_decompress_sparse_dbatch(frames, foff, D, E, **kw)
    else:
        hip.tensor_decompress_seg_sparse_dbatch(frames, foff, D, E, seg_log, **kw)
    torch.cuda.synchronize()
    assert int(res[len(tensors)]) == MARK
    if base is not None and not in_place:
        assert (base.cpu().numpy()[:total] == pc.cat(bases)).all(), "a base that is not the destination is only read"
    return back.cpu().numpy(), res.cpu().tolist()[:len(tensors)]


@pytest.mark.parametrize("form", ["plain", "xor", "sub"])
@pytest.mark.parametrize("E", (1, 2, 4))
def test_composites_give_the_oracles_frames_of_the_models_contents_and_round_trip(hip, checker, E, form):
    from finitestateentropy_amd.api import AutoCodec
    tensors, bases = _pairs(E)
    sizes = [len(t) for t in tensors]
    flat = pc.cat(tensors)
    op = psc.SUB if form == "sub" else psc.XOR
    with_base = bases if form != "plain" else None
    for k, (seg_log, permille, align_log) in enumerate(((None, 500, 0), (10, 500, 6), (11, 1000, 0))):
        F, H = _frames(checker, E, form, seg_log, permille, 0), _frames(checker, E, form, seg_log, permille, 1)
        units = _units_of(_data(E, form), E, seg_log)
        forms = [len(sp.pack_unit(u, permille)) < len(u) for u in units]
        assert form == "plain" or (any(forms) and not all(forms)), "sparse and dense units in one call"
        shift = SHIFTS[k]
        for codec in (0, 1, AutoCodec(20)):
            what = (E, form, seg_log, codec)
            dst, foff, fres, tres, chosen, fcap = run_compress(hip, tensors, with_base, E, op, seg_log, permille, align_log, codec, shift=shift)
            if isinstance(codec, AutoCodec):
                choice = [fmc.expected_choice(len(f), len(h), 20)[0] for f, h in zip(F, H)]
                assert chosen.cpu().tolist() == choice, what
                want = [H[q] if c else F[q] for q, c in enumerate(choice)]
            else:
                assert chosen is None
                want = H if codec else F
            check_frames(want, dst, foff, fres, align_log, fcap, what)
            assert tres.cpu().tolist() == sizes
            for in_place in ((False, True) if with_base is not None else (False,)):
                back, res = run_decompress(hip, dst, foff, tensors, with_base, E, op, seg_log, in_place, shift)
                assert res == sizes, what
                assert (back[:len(flat)] == flat).all() and (back[len(flat):] == FILL).all(), what


@pytest.mark.parametrize("seg_log", [None, 10])
def test_composites_with_a_short_capacity_give_refused_tensors_empty_contents(hip, checker, seg_log):
    E, op = 2, psc.XOR
    tensors, bases = _pairs(E)
    S = [int(x) for x in pc.offsets(tensors)]
    k = 3                                                    # the capacity ends inside tensor 3: it and tensor 4 are refused
    cap = S[k] + 10
    assert S[k + 1] > cap
    empty = checker.frame_compress(np.zeros(0, np.uint8), 0, 1)
    want = []
    for i, d in enumerate(_data(E, "xor")):
        for u in _units_of([d], E, seg_log):
            r, f = checker.frame_compress(sp.pack_unit(u, 500), 0, 1) if i < k else empty
            want.append(f[:r].copy())
    dst, foff, fres, tres, _, fcap = run_compress(hip, tensors, bases, E, op, seg_log, 500, 0, 1, shift=SHIFTS[1], capacity=cap)
    check_frames(want, dst, foff, fres, 0, fcap, seg_log)
    assert tres.cpu().tolist() == [len(t) for t in tensors[:k]] + [GENERIC] * (len(tensors) - k)
    assert all(len(w) == 8 for w in want[-E:])


@pytest.mark.parametrize("seg_log", [None, 10])
def test_a_damaged_frame_and_damaged_contents_leave_the_tensors_slot_alone(hip, checker, seg_log):
    E, op = 2, psc.SUB
    tensors, bases = _pairs(E)
    sizes = [len(t) for t in tensors]
    D = [int(x) for x in pc.offsets(tensors)]
    flat, bflat = pc.cat(tensors), pc.cat(bases)
    dst, foff, fres, _, _, fcap = run_compress(hip, tensors, bases, E, op, seg_log, 500, 0, 0)
    want = _frames(checker, E, "sub", seg_log, 500, 0)
    check_frames(want, dst, foff, fres, 0, fcap, seg_log)
    first = pseg.seg_first(sizes, E, seg_log) if seg_log is not None else list(range(len(tensors) * E + 1))
    # a byte flipped inside a compressed block of tensor 2's first frame: that tensor alone fails, with what the oracle's reader says
    victim = 2
    f = first[victim * E]
    at = 5 + 3 + 40
    bad = want[f].copy()
    assert len(bad) > at + 8
    bad[at] ^= 0x55
    r, _ = checker.frame_decompress(bad, 1024)
    assert r > (1 << 63), "the oracle's reader refuses the damaged frame"
    dst[int(foff[f]) + at] ^= 0x55
    for in_place in (False, True):
        back, res = run_decompress(hip, dst, foff, tensors, bases, E, op, seg_log, in_place)
        assert res == sizes[:victim] + [r - (1 << 64)] + sizes[victim + 1:]
        untouched = bflat if in_place else np.full(D[-1], FILL, np.uint8)
        assert (back[D[victim]:D[victim + 1]] == untouched[D[victim]:D[victim + 1]]).all(), "in place the tensor keeps its old bytes"
        assert (back[:D[victim]] == flat[:D[victim]]).all() and (back[D[victim + 1]:D[-1]] == flat[D[victim + 1]:]).all() and (back[D[-1]:] == FILL).all()
    # damaged CONTENTS in intact frames: the oracle's frames of every refusal of the reader rule, each in the place of a unit of tensor 0
    units = _units_of(_data(E, "sub"), E, seg_log)
    q = first[2] - 1                                         # plane 1 of tensor 0, or its last segment
    n_unit = len(units[q])
    victim_unit = sp.with_density(n_unit, n_unit // 9, 12)
    victim_unit[-1] = 0
    assert n_unit % 8, "a partial last mask byte"
    for name, content, _ in sp.damaged_contents(victim_unit):
        frames = [w for w in want]
        r, fr = checker.frame_compress(content, 0, 0)
        frames[q] = fr[:r].copy()
        off = [int(x) for x in pc.offsets(frames)]
        for in_place in (False, True):
            back, res = run_decompress(hip, _dev(pc.cat(frames)), _i64(off), tensors, bases, E, op, seg_log, in_place)
            assert res == [CORRUPT] + sizes[1:], name
            untouched = bflat if in_place else np.full(D[-1], FILL, np.uint8)
            assert (back[:D[1]] == untouched[:D[1]]).all(), (name, "the slot is not written; in place it keeps its old bytes")
            assert (back[D[1]:D[-1]] == flat[D[1]:]).all() and (back[D[-1]:] == FILL).all(), name


@pytest.mark.parametrize("E", (1, 2, 4))
def test_a_threshold_under_which_nothing_qualifies_gives_the_existing_composites_bit_for_bit(hip, E):
    from finitestateentropy_amd.api import AutoCodec
    sizes = [E * 3000 + 1, 0, E * 1024, 7, E * 2100]
    tensors, bases = pc.random_tensors(sizes, 300 + E), pc.random_tensors(sizes, 400 + E)
    for data in (tensors, psc.delta_all(tensors, bases, E, psc.XOR), psc.delta_all(tensors, bases, E, psc.SUB)):
        assert all(u.any() or len(u) < 2 for u in _units_of(data, E, 10)), "no unit is all zero: permille 0 admits none"
    S = pc.offsets(tensors)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))

    def same(a, b, what):
        torch.cuda.synchronize()
        for x, y in zip(a[1:4], b[1:4]):
            assert torch.equal(x, y), what
        assert (a[4] is None and b[4] is None) or torch.equal(a[4], b[4]), what
        off, res = a[1].cpu().tolist(), a[2].cpu().tolist()
        assert min(res) >= 8
        for q in range(len(res)):
            assert torch.equal(a[0][off[q]:off[q] + res[q]], b[0][off[q]:off[q] + res[q]]), (what, q)
    for align_log in (0, 6):
        for codec in (0, 1):
            a = hip.tensor_compress_dbatch(src, S, E, 0, codec, align_log=align_log) + (None,)
            same(a, hip.tensor_compress_sparse_dbatch(src, S, E, 0, codec=codec, block_size_id=0, align_log=align_log), ("plain", codec))
            a = hip.tensor_compress_delta_dbatch(src, base, S, E, 0, codec, align_log=align_log, delta_op=1) + (None,)
            same(a, hip.tensor_compress_sparse_dbatch(src, S, E, 0, base=base, codec=codec, block_size_id=0, align_log=align_log, delta_op=1), ("sub", codec))
        a = hip.tensor_compress_mixed_dbatch(src, S, E, base, None, 20, 0, align_log=align_log)
        same(a, hip.tensor_compress_sparse_dbatch(src, S, E, 0, base=base, codec=AutoCodec(20), block_size_id=0, align_log=align_log), "mixed")
        for codec in (1, AutoCodec(20)):
            a = hip.tensor_compress_seg_dbatch(src, S, E, 10, base=base, codec=codec, block_size_id=0, align_log=align_log, delta_op=1)
            same(a, hip.tensor_compress_seg_sparse_dbatch(src, S, E, 10, 0, base=base, codec=codec, block_size_id=0, align_log=align_log, delta_op=1), ("seg", codec))
    # ... and the sparse reader reads the frames of the existing writer: all contents are dense
    a = hip.tensor_compress_delta_dbatch(src, base, S, E, 0, 0, delta_op=1)
    back, res = hip.tensor_decompress_sparse_dbatch(a[0], a[1], S, E, base=base, delta_op=1)
    assert res.cpu().tolist() == sizes and torch.equal(back[:int(S[-1])], src)


def test_the_eight_sums_of_the_size_table_on_the_device(hip):
    old, new = pdc.bf16_update_pair()
    src, base = _dev(new), _dev(old)
    S = np.array([0, new.size], np.uint64)
    got = {}
    for name, op in (("xor", 0), ("sub", 1)):
        for codec in (0, 1):
            dense = hip.tensor_compress_delta_dbatch(src, base, S, 2, 5, codec, delta_op=op)[2]
            sparse = hip.tensor_compress_sparse_dbatch(src, S, 2, 500, base=base, codec=codec, block_size_id=5, delta_op=op)[2]
            got[(name, codec)] = (int(dense.sum()), int(sparse.sum()))
    print(got)
    assert got == sp.TABLE


def test_sparse_compress_and_decompress_in_one_hip_graph(hip, checker):
    """one captured graph -- a single stream, a linear chain -- holding tensor_compress_seg_sparse_dbatch and then
    tensor_decompress_seg_sparse_dbatch in place over the base; replayed twice, the source changed in between"""
    E, codec, ALIGN, seg_log, op, permille = 2, 1, 4, 10, psc.SUB, 500
    shapes, bases = _pairs(E)
    sizes = [len(t) for t in shapes]
    n, S = len(sizes), pc.offsets(shapes)
    total = int(S[-1])
    first = pseg.seg_first(sizes, E, seg_log)
    nseg = first[-1]
    blocks = hip.planes_block_bound(total, n, E, 0)
    fcap = hip.frame_packed_bound(total, nseg, blocks, ALIGN)
    wsize, rsize = hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize, hip.lib.FSEHIP_frame_decompress_packed_dbatch_workspaceSize
    wsize.restype = rsize.restype = C.c_size_t
    head = hip.sparse_workspace_bound(total, nseg)
    wws = torch.empty(head + int(wsize(C.c_size_t(nseg), C.c_size_t(blocks), C.c_uint(0), C.c_int(codec))), dtype=torch.uint8, device="cuda")
    rws = torch.empty(head + int(rsize(C.c_size_t(nseg), C.c_size_t(blocks))), dtype=torch.uint8, device="cuda")
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    base = _dev(pc.cat(bases))
    soff, sf = _i64(S), _i64(first)
    frames, back, planes, planes2, contents, contents2 = (_filled(fcap),) + tuple(_filled(total) for _ in range(5))
    foff, so, so2, coff, coff2 = (torch.zeros(nseg + 1, dtype=torch.int64, device="cuda") for _ in range(5))
    fres, sres, cres = (torch.zeros(nseg, dtype=torch.int64, device="cuda") for _ in range(3))
    poff, poff2 = (torch.zeros(n * E + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    psz = torch.zeros(n * E, dtype=torch.int64, device="cuda")
    tres, rres = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))

    def work():
        hip.tensor_compress_seg_sparse_dbatch(src, soff, E, seg_log, permille, sf, n_segments=nseg, base=base, codec=codec, block_size_id=0, dst=frames, dst_capacity=fcap,
                                              max_total_blocks=blocks, align_log=ALIGN, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes,
                                              plane_offsets=poff, seg_offsets=so, contents=contents, content_offsets=coff, workspace=wws, delta_op=op)
        back[:total].copy_(base)
        hip.tensor_decompress_seg_sparse_dbatch(frames, foff, soff, E, seg_log, sf, n_segments=nseg, base=back, dst=back, dst_capacity=total, max_total_blocks=blocks,
                                                contents=contents2, contents_capacity=total, content_offsets=coff2, content_results=cres, planes=planes2,
                                                planes_capacity=total, seg_offsets=so2, seg_results=sres, plane_offsets=poff2, plane_sizes=psz, workspace=rws,
                                                results=rres, delta_op=op)

    def source(seed):
        return pc.random_tensors(sizes, seed) if seed % 2 else [np.asarray(t) for t in shapes]
    src.copy_(_dev(pc.cat(source(0)))); work(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    seen = []
    for trial in (1, 2):
        tensors = source(trial)
        seen.append(pc.cat(tensors))
        src.copy_(_dev(seen[-1]))
        for t in (frames, back):
            t.fill_(FILL)
        for t in (foff, fres, tres, rres):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        units = _units_of(psc.delta_all(tensors, bases, E, op), E, seg_log)
        want = [f[:r].copy() for u in units for r, f in [checker.frame_compress(sp.pack_unit(u, permille), 0, codec)]]
        check_frames(want, frames, foff, fres, ALIGN, fcap, trial)
        assert tres.cpu().tolist() == rres.cpu().tolist() == sizes
        out = back.cpu().numpy()
        assert (out[:total] == seen[-1]).all() and (out[total:] == FILL).all()
    assert not (seen[0] == seen[1]).all()


# ---------------------------------------------------------------------------------------------------------------- the user-facing pair
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_compress_tensors_with_sparse_planes_round_trips_mixed_dtypes(hip):
    from finitestateentropy_amd.api import AutoCodec, DeltaBase, SparsePlanes
    g = torch.Generator(device="cuda").manual_seed(5)
    old = [torch.randn(3000, 7, device="cuda", generator=g).to(torch.bfloat16), torch.randn(5001, device="cuda", generator=g),
           torch.randint(0, 255, (4099,), device="cuda", generator=g, dtype=torch.uint8), torch.randn(1200, device="cuda", generator=g, dtype=torch.float64),
           torch.zeros(0, device="cuda", dtype=torch.float16)]
    new = [(o.float() * (1 + 1e-2 * (torch.rand(o.shape, device="cuda", generator=g) < 0.1))).to(o.dtype) if o.is_floating_point() else o.clone() for o in old]
    new[2][::9] += 1
    assert all(n.dtype == o.dtype for n, o in zip(new, old)) and not _bits(new[0], old[0])
    dense = hip.compress_tensors(new, codec=1, base=DeltaBase(old, "sub"))
    for codec in (SparsePlanes(1), SparsePlanes(0, 1000), SparsePlanes(AutoCodec(20), 300)):
        obj = hip.compress_tensors(new, codec=codec, base=DeltaBase(old, "sub"))
        assert obj.sparse_permille == codec.permille and obj.codec == codec and obj.delta and obj.delta_op == "sub" and obj.segment_log is None
        assert ("codecs" in obj.groups[0]) == isinstance(codec.codec, AutoCodec)
        back = hip.decompress_tensors(obj, base=old)
        assert all(_bits(b, n) and b.dtype == n.dtype and b.shape == n.shape for b, n in zip(back, new))
        seg = hip.compress_tensors_segmented(new, 12, codec=codec, block_size_id=0, base=DeltaBase(old, "sub"))
        assert seg.sparse_permille == codec.permille and seg.segment_log == 12
        back = hip.decompress_tensors(seg, base=DeltaBase(old, "sub"))
        assert all(_bits(b, n) for b, n in zip(back, new))
        with pytest.raises(ValueError, match="sparse"):
            hip.decompress_tensor_windows(seg, [None] * len(new), base=old)
        with pytest.raises(ValueError, match="sparse"):
            hip.patch_tensor_windows(seg, new, [None] * len(new), base=old)
    sparse = hip.compress_tensors(new, codec=SparsePlanes(1), base=DeltaBase(old, "sub"))
    print("Huff0 frames of the update: dense %d bytes, sparse %d" % (dense.nbytes, sparse.nbytes))
    assert sparse.nbytes < dense.nbytes
    # without a base, and the codecs of an AutoCodec object given again
    plain = hip.compress_tensors(new, codec=SparsePlanes(0))
    assert all(_bits(b, n) for b, n in zip(hip.decompress_tensors(plain), new))
    first = hip.compress_tensors(new, codec=SparsePlanes(AutoCodec(20)), base=old)
    again = hip.compress_tensors(new, codec=first, base=old)
    assert again.sparse_permille == 500 and all(torch.equal(a["frames"], b["frames"]) and torch.equal(a["codecs"], b["codecs"]) for a, b in zip(first.groups, again.groups))
