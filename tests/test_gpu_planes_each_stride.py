"""Strides in the estimate and a stride per tensor on the device (FSEHIP_planes_estimate_stride_dbatch, the six FSEHIP_*_each_stride_dbatch
calls, compress_tensors_each(..., strides=...)) -- bit for bit against the integer model of planes_each_stride_corpus.py and byte for byte
against the existing dedicated device calls run per transform and per stride on the same tensors.  Tile T = 32 KB, run = 1024 elements,
block-size id 0 wherever frames are involved.  Outputs are pre-filled and have a spare entry or a tail behind them that must stay as it was;
sources, bases, transforms and strides must come back unchanged."""
import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_each_corpus as pe
import planes_each_stride_corpus as pes
import planes_estimate_corpus as pest
import planes_stride_corpus as psc
from planes_corpus import GENERIC, TILE
from planes_each_stride_corpus import PLAIN, PRED, SUB, XOR
from planes_estimate_corpus import NO_CHOICE, ONES

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, 0xF9
SHIFTS = ((0, 0, 0), (1, 5, 9), (8, 15, 3), (3, 2, 13))     # source, base, destination: each off 16-byte alignment by an amount of its own
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def _filled(n, shift=0, content=None):
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def _only_read(buf, content, what):
    host = buf.cpu().numpy()
    assert (host[:len(content)] == content).all() and (host[len(content):] == FILL).all(), what + " is only read"


def counts():
    """the element counts of the issue: around a run, 1024 + S for every stride, the phase-restart case"""
    return [1023, 1024, 1025] + [1024 + S for S in (2, 3, 5, 8)] + [4 * 1024 + 7]


def _walk(rng, m, E):
    """m elements of E bytes in S = 1 + m % 4 interleaved slow walks: strides differ in cost"""
    ch = 1 + m % 4
    v = np.cumsum(rng.integers(-3, 4, (m // ch + 1, ch)), axis=0) + 1000 * (1 + np.arange(ch))
    return v.reshape(-1)[:m].astype(np.uint64).astype(psc._U[E]).view(np.uint8).copy()


def _corpus(E):
    """-> (tensors, bases, tiny): tensors of 0 .. 40 bytes; the counts of the issue as whole elements and with n mod E != 0; the list padded to a
    tile, 130 tiny tensors that share it (tensors[tiny[0]:tiny[1]]) and a tensor of three tiles and 5 bytes beside them; a constant tensor and
    a tensor equal to its base.  Walks in interleaved channels and random bytes alternate; the bases are near copies or random"""
    if E not in _CACHE:
        rng = np.random.default_rng(1100 + E)
        tensors = [rng.integers(0, 256, n, dtype=np.uint8) for n in range(41)]
        for k, c in enumerate(counts()):
            tensors.append(_walk(rng, c, E))
            tensors.append(np.concatenate([_walk(rng, c, E), rng.integers(0, 256, 1 + k % (E - 1), dtype=np.uint8)]) if E > 1 else rng.integers(0, 256, c, dtype=np.uint8))
        at = sum(len(t) for t in tensors)
        tensors.append(rng.integers(0, 256, -at % TILE, dtype=np.uint8))          # the tiny ones start a tile ...
        tiny = (len(tensors), len(tensors) + 130)
        tensors += [_walk(rng, int(n) // E, E) if k % 2 else rng.integers(0, 256, int(n), dtype=np.uint8) for k, n in enumerate(rng.integers(1, 41, 130))]
        assert sum(len(t) for t in tensors[tiny[0]:tiny[1]]) < TILE // 4, "... and share it"
        tensors.append(np.concatenate([_walk(rng, 3 * TILE // E, E), np.arange(1, 6, dtype=np.uint8)]))
        tensors.append(np.full(TILE + 2 * E + 1, 0x3C, np.uint8))
        same = _walk(rng, (TILE + 48) // E, E)
        tensors.append(same)
        bases = []
        for k, t in enumerate(tensors):
            b = rng.integers(0, 256, len(t), dtype=np.uint8)
            if k % 3 == 0 and len(t):
                b = t.copy()
                b[rng.integers(0, len(t), max(len(t) // 50, 1))] ^= 1
            bases.append(b)
        bases[-1] = same.copy()
        _CACHE[E] = (tensors, bases, tiny)
    return _CACHE[E]


# ---------------------------------------------------------------------------------------------------------------- the estimate
def _cand(E, i, kind):
    """the model's (plane bits, estimate) of tensor i of the corpus under PLAIN, XOR, SUB or ("S", stride): computed once, the runs below compose them"""
    key = ("cand", E, i, kind)
    if key not in _CACHE:
        tensors, bases, _ = _corpus(E)
        planes = pes.stride_planes(tensors[i], E, kind[1]) if isinstance(kind, tuple) else pest.candidate_planes(tensors[i], bases[i], E, kind)
        _CACHE[key] = ([pest.plane_bits(p) for p in planes], pest.est_bytes(planes))
    return _CACHE[key]


def composed(E, mask, smask, margin, refused=()):
    """the six outputs of the call on the corpus from the cached candidates, by the rules of planes_each_stride_corpus.py"""
    tensors, _, _ = _corpus(E)
    bits, est, choice, res, sest, strides = [], [], [], [], [], []
    for i, t in enumerate(tensors):
        if i in refused:
            bits += [ONES] * (4 * E); est += [ONES] * 4; choice.append(NO_CHOICE); res.append(GENERIC); sest += [ONES] * 8; strides.append(pes.NO_STRIDE)
            continue
        mine_s = [_cand(E, i, ("S", S))[1] if mask & 2 and (smask >> (S - 1)) & 1 else ONES for S in pes.STRIDES]
        best = pes.choose_stride(mine_s, smask, margin) if mask & 2 else 1
        mine = []
        for c in range(4):
            b, e = _cand(E, i, ("S", best) if c == PRED else c) if (mask >> c) & 1 else ([ONES] * E, ONES)
            bits += b
            mine.append(e)
        est += mine
        choice.append(pest.choose(mine, mask, margin))
        res.append(len(t))
        sest += mine_s
        strides.append(best)
    return bits, est, choice, res, sest, strides


def run_estimate(hip, tensors, bases, E, mask, smask, margin=50, capacity=None, shift=(0, 0, 0), offsets=None, with_sest=True):
    S = pc.offsets(tensors) if offsets is None else np.asarray(offsets, np.uint64)
    n = len(S) - 1
    flat = pc.cat(tensors)
    total = len(flat)
    src = _filled(total, shift[0], flat)
    bflat = None if bases is None else pc.cat(bases)
    base = None if bases is None else _filled(total, shift[1], bflat)
    pb = torch.full((n * 4 * E + 1,), -7, dtype=torch.int64, device="cuda")
    eb = torch.full((n * 4 + 1,), -7, dtype=torch.int64, device="cuda")
    ch = torch.full((n + 1,), MARK, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 1,), MARK, dtype=torch.uint8, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    seb = torch.full((n * 8 + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_estimate_stride_dbatch(src[:total], S, E, mask, smask, margin, base=None if base is None else base[:total], capacity=capacity, plane_bits=pb, est_bytes=eb,
                                      choice=ch, results=res, stride_est_bytes=seb, strides=st)
    torch.cuda.synchronize()
    assert int(pb[-1]) == -7 and int(eb[-1]) == -7 and int(ch[-1]) == MARK and int(res[-1]) == -7 and int(seb[-1]) == -7 and int(st[-1]) == MARK, "the entry behind every output"
    _only_read(src, flat, "the source")
    if base is not None:
        _only_read(base, bflat, "the base")
    u = lambda t: [x & ONES for x in t.cpu().tolist()[:-1]]
    return u(pb), u(eb), ch.cpu().tolist()[:-1], res.cpu().tolist()[:-1], u(seb), st.cpu().tolist()[:-1]


def check(got, want, what):
    for name, g, w in zip(("plane bits", "estimates", "choice", "results", "stride estimates", "strides"), got, want):
        assert len(g) == len(w), (what, name)
        bad = [k for k in range(len(w)) if g[k] != w[k]]
        assert not bad, (what, name, bad[:8], [g[k] for k in bad[:4]], [w[k] for k in bad[:4]])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_estimate_over_strides_against_the_model(hip, E):
    tensors, bases, tiny = _corpus(E)
    sizes = [len(t) for t in tensors]
    assert all(c * E in sizes for c in counts()) and (E == 1 or all(any(c * E < s < (c + 1) * E for s in sizes) for c in counts())) and set(range(41)) <= set(sizes)
    full = composed(E, 15, 0xFF, 50)
    if E == 2:                                                  # the composition above is the model's own, once on a part that holds every kind of tensor
        k = tiny[0] - 18
        assert tuple(x[len(x) // len(tensors) * k:] for x in full) == pes.estimate_stride_model(tensors[k:], E, 15, 0xFF, bases[k:], 50)
    assert len(set(full[5])) >= 4, "the corpus has tensors of several channel counts: %r" % sorted(set(full[5]))
    for k, shift in enumerate(SHIFTS):
        check(run_estimate(hip, tensors, bases, E, 15, 0xFF, 50, shift=shift), full, (E, shift))
    for S in pes.STRIDES:                                        # every single-bit mask: that stride's numbers in the PRED slots
        got = run_estimate(hip, tensors, None, E, 3, 1 << (S - 1), (0, 50, 1000)[S % 3], shift=SHIFTS[S % 4])
        check(got, composed(E, 3, 1 << (S - 1), (0, 50, 1000)[S % 3]), (E, "stride", S))
        assert got[5] == [S] * len(tensors)
    # the one-value fast path beside stride candidates: the constant tensor and tensor == base under XOR | SUB | PRED
    got = run_estimate(hip, tensors, bases, E, 14, 0x2D, 0, shift=SHIFTS[2])
    check(got, composed(E, 14, 0x2D, 0), (E, "xor | sub | pred"))
    n = len(tensors)
    assert got[1][4 * (n - 1) + XOR] == got[1][4 * (n - 1) + SUB] == 0 and got[2][n - 1] == XOR, "tensor == base: the delta planes are all zeros"
    check(run_estimate(hip, tensors, bases, E, 15, 0x0F, 1000, shift=SHIFTS[1]), composed(E, 15, 0x0F, 1000), (E, "margin 1000"))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_stride_one_is_the_existing_estimate(hip, E):
    tensors, bases, _ = _corpus(E)
    S = pc.offsets(tensors)
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    n = len(tensors)
    for mask, margin in ((15, 50), (3, 0), (13, 50), (2, 300)):
        old = hip.planes_estimate_dbatch(src, S, E, mask, margin, base=base)
        new = hip.planes_estimate_stride_dbatch(src, S, E, mask, 1, margin, base=base)
        assert all(torch.equal(a, b) for a, b in zip(old, new[:4])), "strideMask 1: every shared output is that of the existing call"
        assert new[5].cpu().tolist() == [1] * n
        seb = new[4].cpu().tolist()
        assert all(x == -1 for k, x in enumerate(seb) if k % 8 or not mask & 2)
        if mask & 2:
            assert seb[0::8] == old[1].cpu().tolist()[PRED::4], "stride 1's entries: the existing PRED numbers"
    old = hip.planes_estimate_dbatch(src, S, E, 3, 50)
    new = hip.planes_estimate_stride_dbatch(src, S, E, 3, 0xFF, 50)
    assert new[4].cpu().tolist()[0::8] == old[1].cpu().tolist()[PRED::4], "... under every strideMask"


@pytest.mark.parametrize("E", pc.ELEMS)
def test_estimate_refusals(hip, E):
    tensors, bases, _ = _corpus(E)
    S = [int(x) for x in pc.offsets(tensors)]
    k = next(i for i, t in enumerate(tensors) if len(t) == 1025 * E)
    for cap in (S[k] + 100, S[k + 1], S[6], 0):                 # a short capacity: the tensors behind it are refused, all-ones and 0xFF
        refused = {i for i in range(len(tensors)) if S[i + 1] > cap}
        check(run_estimate(hip, tensors, bases, E, 15, 0x0F, 50, capacity=cap, shift=SHIFTS[1]), composed(E, 15, 0x0F, 50, refused), (E, cap))
    rng = np.random.default_rng(43)
    flat = rng.integers(0, 256, 320, dtype=np.uint8)
    offsets = [0, 100, 60, 200, 300, 370]                       # slot 1 decreases, slot 4 ends behind the capacity
    units = [flat[a:b] if a <= b <= 320 else flat[:0] for a, b in zip(offsets, offsets[1:])]
    want = pes.estimate_stride_model(units, E, 3, 0xFF, None, 50, capacity=320, offsets=offsets)
    got = run_estimate(hip, [flat], None, E, 3, 0xFF, 50, capacity=320, offsets=offsets)
    check(got, want, E)
    assert got[3] == [100, GENERIC, 140, 100, GENERIC] and got[5][1] == got[5][4] == 0xFF and got[4][8:16] == [ONES] * 8


def test_the_interleaved_corpora_choose_their_channel_count(hip):
    for name, (E, t, stride, tr) in pes.table(1 << 16).items():
        if stride == 1:
            continue
        src = _dev(t)
        _, eb, ch, res, seb, st = hip.planes_estimate_stride_dbatch(src, np.array([0, len(t)], np.uint64), E, 3, 0xFF, 50)
        want = [pest.est_bytes(pes.stride_planes(t, E, S)) for S in pes.STRIDES]
        print("%-20s plain %d, strides 1 .. 8 %s" % (name, int(eb[0]), seb.cpu().tolist()))
        assert seb.cpu().tolist() == want and st.cpu().tolist() == [stride] and ch.cpu().tolist() == [tr] and int(eb[1]) == want[stride - 1], name


def test_estimate_in_a_hip_graph_replayed_over_changed_sources(hip):
    E, mask, smask, margin = 2, 3, 0x0F, 50
    sizes = [0, 3 * TILE + 4, 778, TILE, 2 * TILE + 6]
    n, S = len(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)

    def load(seed):
        rng = np.random.default_rng(seed)
        ts = [_walk(rng, s // E + (seed + k) % 4, E)[:s] for k, s in enumerate(sizes)]        # (the channel count follows the element count: it changes with the seed)
        src.copy_(_dev(pc.cat(ts)))
        return pes.estimate_stride_model(ts, E, mask, smask, None, margin)
    src = torch.zeros(int(S[-1]), dtype=torch.uint8, device="cuda")
    soff = _i64(S)
    pb, eb, res, seb = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n * 4 * E, n * 4, n, n * 8))
    ch, st = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hip.planes_estimate_stride_workspace_bound(n, E, mask, smask), dtype=torch.uint8, device="cuda")

    def work():
        hip.planes_estimate_stride_dbatch(src, soff, E, mask, smask, margin, plane_bits=pb, est_bytes=eb, choice=ch, results=res, stride_est_bytes=seb, strides=st, workspace=ws)

    def outputs():
        torch.cuda.synchronize()
        u = lambda t: [x & ONES for x in t.cpu().tolist()]
        return u(pb), u(eb), ch.cpu().tolist(), res.cpu().tolist(), u(seb), st.cpu().tolist()
    want = load(0); work()
    check(outputs(), want, "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    seen = [want]
    for seed in (101, 202):
        want = load(seed)
        assert want[5] not in [w[5] for w in seen], "the changed source has other strides"
        seen.append(want)
        for t in (pb, eb, res, seb, ch, st):
            t.fill_(3)
        ws.fill_(0x5A)
        g.replay()
        check(outputs(), want, ("replay", seed))


# ---------------------------------------------------------------------------------------------------------------- split and merge
def _kinds(E, lead):
    """the transforms and strides of the corpus: the walk over all 121 ordered pairs of the eleven kinds, started `lead` entries in"""
    tensors, _, tiny = _corpus(E)
    tr, st = pes.cycle_transforms_and_strides(len(tensors), lead)
    pairs = set(zip(zip(tr[tiny[0]:tiny[1] - 1], st[tiny[0]:tiny[1] - 1]), zip(tr[tiny[0] + 1:tiny[1]], st[tiny[0] + 1:tiny[1]])))
    assert len(pairs) == 121, "every pair of neighbours occurs inside the shared tile"
    return tr, st


def _dedicated(hip, E):
    """the planes of the dedicated splits on the corpus, each run once: PLAIN, XOR, SUB and ("S", stride) -> (planes, plane offsets, results)"""
    key = ("dedicated", E)
    if key not in _CACHE:
        tensors, bases, _ = _corpus(E)
        S = pc.offsets(tensors)
        src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
        runs = {PLAIN: hip.planes_split_dbatch(src, S, E), XOR: hip.planes_split_xor_dbatch(src, base, S, E), SUB: hip.planes_split_xor_dbatch(src, base, S, E, delta_op=1)}
        for s in pes.STRIDES:
            runs[("S", s)] = hip.planes_split_pred_stride_dbatch(src, S, E, s)
        torch.cuda.synchronize()
        _CACHE[key] = {k: (p.cpu().numpy()[:int(S[-1])], o.cpu().tolist(), r.cpu().tolist()) for k, (p, o, r) in runs.items()}
    return _CACHE[key]


def run_split(hip, tensors, bases, E, transforms, strides, capacity=None, shift=(0, 0, 0)):
    S = pc.offsets(tensors)
    n, total = len(S) - 1, sum(len(t) for t in tensors)
    src, planes = _filled(total, shift[0], pc.cat(tensors)), _filled(total, shift[2])
    base = None if bases is None else _filled(total, shift[1], pc.cat(bases))
    poff = torch.full((n * E + 2,), -7, dtype=torch.int64, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tr = _filled(n, 1, np.asarray(transforms, np.uint8))
    st = None if strides is None else _filled(n, 3, np.asarray(strides, np.uint8))
    hip.planes_split_each_stride_dbatch(src[:total], S, E, tr[:n], None if st is None else st[:n], base=None if base is None else base[:total], capacity=capacity,
                                        planes=planes, plane_offsets=poff, results=res)
    torch.cuda.synchronize()
    assert int(poff[n * E + 1]) == -7 and int(res[n]) == -7
    _only_read(src, pc.cat(tensors), "the source")
    _only_read(tr, np.asarray(transforms, np.uint8), "the transforms")
    if st is not None:
        _only_read(st, np.asarray(strides, np.uint8), "the strides")
    if base is not None:
        _only_read(base, pc.cat(bases), "the base")
    return planes.cpu().numpy(), poff.cpu().tolist()[:n * E + 1], res.cpu().tolist()[:n]


def check_split(got, tensors, bases, E, transforms, strides, capacity=None):
    out, poff, res = got
    want, written, P, wres = pes.split_each_stride_model(tensors, bases, E, transforms, strides, capacity)
    assert poff == P and res == wres
    total = len(want)
    assert (out[:total][written] == want[written]).all(), np.nonzero((out[:total] != want) & written)[0][:8]
    outside = np.ones(len(out), bool)
    outside[:total] = ~written
    assert (out[outside] == FILL).all(), ("bytes outside the accepted tensors' planes", np.nonzero((out != FILL) & outside)[0][:8])


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_each_stride_byte_for_byte(hip, E):
    tensors, bases, tiny = _corpus(E)
    S = [int(x) for x in pc.offsets(tensors)]
    ded = _dedicated(hip, E)
    for k, lead in enumerate((0, 47, 93)):
        tr, st = _kinds(E, lead)
        got = run_split(hip, tensors, bases, E, tr, st, shift=SHIFTS[k])
        check_split(got, tensors, bases, E, tr, st)
        for i in range(len(tensors)):                           # the dedicated call of every tensor's transform and stride
            d = ded[("S", st[i]) if tr[i] == PRED else tr[i]]
            assert got[1] == d[1] and got[2] == d[2] and (got[0][S[i]:S[i + 1]] == d[0][S[i]:S[i + 1]]).all(), (lead, i, tr[i], st[i])
    # strides NULL: the _each_ call
    tr, _ = _kinds(E, 5)
    got = run_split(hip, tensors, bases, E, tr, None, shift=SHIFTS[3])
    planes, poff, res = hip.planes_split_each_dbatch(_dev(pc.cat(tensors)), pc.offsets(tensors), E, tr, base=_dev(pc.cat(bases)))
    assert (got[0][:S[-1]] == planes.cpu().numpy()[:S[-1]]).all() and got[1] == poff.cpu().tolist() and got[2] == res.cpu().tolist()


@pytest.mark.parametrize("E", pc.ELEMS)
def test_split_each_stride_refusals_and_a_short_capacity(hip, E):
    tensors, bases, tiny = _corpus(E)
    n = len(tensors)
    S = [int(x) for x in pc.offsets(tensors)]
    tr, st = _kinds(E, 11)
    big = n - 3                                                 # the tensor of three tiles
    hit = [43, tiny[0] + 7, tiny[0] + 8, tiny[0] + 60, big]
    for j, i in enumerate(hit):                                 # stride bytes 0 and 9 (and 255) on PRED tensors: refused alone
        tr[i], st[i] = PRED, (0, 9, 255)[j % 3]
    for i in range(n):                                          # garbage stride bytes on the others: ignored
        if tr[i] != PRED:
            st[i] = (0, 9, 77, 255)[i % 4]
    got = run_split(hip, tensors, bases, E, tr, st, shift=SHIFTS[1])
    check_split(got, tensors, bases, E, tr, st)
    assert [r == GENERIC for r in got[2]] == [i in hit for i in range(n)] and all((got[0][S[i]:S[i + 1]] == FILL).all() for i in hit)
    # XOR and SUB with a NULL base are refused per tensor, as ever
    tr, st = _kinds(E, 3)
    got = run_split(hip, tensors, None, E, tr, st, shift=SHIFTS[2])
    check_split(got, tensors, None, E, tr, st)
    assert [r == GENERIC for r in got[2]] == [t >= XOR for t in tr]
    k = next(i for i, t in enumerate(tensors) if len(t) == 1025 * E)
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):
        tr, st = _kinds(E, 29)
        got = run_split(hip, tensors, bases, E, tr, st, capacity=cap, shift=SHIFTS[3])
        check_split(got, tensors, bases, E, tr, st, cap)
        first = next(i for i in range(n) if S[i + 1] > cap)
        assert got[2][first:] == [GENERIC] * (n - first) and (got[0][S[first]:] == FILL).all()


def run_merge(hip, E, planes_buf, poff, psizes, D, transforms, strides, bases=None, in_place=False, capacity=None, shift=(0, 0, 0)):
    n, room = len(D) - 1, int(D[-1])
    planes = _filled(len(planes_buf), shift[0], planes_buf)
    content = None if bases is None else pc.cat(bases)
    dst = _filled(room, shift[2], content if in_place else None)
    base = None if bases is None else dst if in_place else _filled(room, shift[1], content)
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tr = _filled(n, 1, np.asarray(transforms, np.uint8))
    st = None if strides is None else _filled(n, 3, np.asarray(strides, np.uint8))
    out, _ = hip.planes_merge_each_stride_dbatch(planes[:max(len(planes_buf), 1)], _i64(poff), _i64(psizes), np.asarray(D, np.uint64), E, tr[:n],
                                                 None if st is None else st[:n], base=None if base is None else base[:room], dst=dst,
                                                 capacity=room if capacity is None else capacity, results=res)
    torch.cuda.synchronize()
    assert int(res[n]) == -7 and out.data_ptr() == dst.data_ptr()
    _only_read(planes, planes_buf, "the planes")
    if base is not None and not in_place:
        _only_read(base, content, "the base")
    return dst.cpu().numpy(), res.cpu().tolist()[:n]


@pytest.mark.parametrize("E", pc.ELEMS)
def test_merge_each_stride_is_the_exact_inverse(hip, E):
    tensors, bases, tiny = _corpus(E)
    n = len(tensors)
    S = [int(x) for x in pc.offsets(tensors)]
    flat = pc.cat(tensors)
    for k, lead in enumerate((0, 47, 93)):
        tr, st = _kinds(E, lead)
        planes, _, P, _ = pes.split_each_stride_model(tensors, bases, E, tr, st)
        psz = [P[j + 1] - P[j] for j in range(n * E)]
        for in_place in (False, True):                          # in place: over the base, XOR / SUB tensors beside PRED ones
            out, res = run_merge(hip, E, planes, P[:-1], psz, S, tr, st, bases, in_place, shift=SHIFTS[(k + in_place) % 4])
            assert res == [len(t) for t in tensors] and (out[:S[-1]] == flat).all() and (out[S[-1]:] == FILL).all(), (lead, in_place)
    # refusals in place: stride bytes 0 and 9 on PRED tensors keep their old bytes, their neighbours are rebuilt; garbage on the others is ignored
    tr, st = _kinds(E, 11)
    planes, _, P, _ = pes.split_each_stride_model(tensors, bases, E, tr, st)
    psz = [P[j + 1] - P[j] for j in range(n * E)]
    pred = [i for i in range(n) if tr[i] == PRED]
    hit = [pred[5], next(i for i in pred if tiny[0] + 3 < i < tiny[1]), next(i for i in pred if i >= tiny[0] + 40), pred[-1]]
    given = [(0, 9)[hit.index(i) % 2] if i in hit else s if tr[i] == PRED else (0, 9, 77, 255)[i % 4] for i, s in enumerate(st)]
    out, res = run_merge(hip, E, planes, P[:-1], psz, S, tr, given, bases, True, shift=SHIFTS[3])
    for i in range(n):
        if i in hit:
            assert res[i] == GENERIC and (out[S[i]:S[i + 1]] == bases[i]).all(), i
        else:
            assert res[i] == len(tensors[i]) and (out[S[i]:S[i + 1]] == tensors[i]).all(), i
    assert (out[S[-1]:] == FILL).all()
    # strides NULL: the _each_ call, on planes split at stride 1
    tr, _ = _kinds(E, 5)
    planes, _, P, _ = pe.split_each_model(tensors, bases, E, tr)
    out, res = run_merge(hip, E, planes, P[:-1], [P[j + 1] - P[j] for j in range(n * E)], S, tr, None, bases, shift=SHIFTS[1])
    assert res == [len(t) for t in tensors] and (out[:S[-1]] == flat).all()
    # a short capacity
    tr, st = _kinds(E, 29)
    planes, _, P, _ = pes.split_each_stride_model(tensors, bases, E, tr, st)
    cap = S[n - 3] + 5
    out, res = run_merge(hip, E, planes, P[:-1], [P[j + 1] - P[j] for j in range(n * E)], S, tr, st, bases, False, capacity=cap, shift=SHIFTS[2])
    first = next(i for i in range(n) if S[i + 1] > cap)
    assert res[first:] == [GENERIC] * (n - first) and (out[S[first]:] == FILL).all() and (out[:S[first]] == flat[:S[first]]).all()


# ---------------------------------------------------------------------------------------------------------------- composites
def _small(E):
    """a short list for the composites: empty, tiny, odd, more than a run, a tile and more -- interleaved walks and random bytes; bases near or random"""
    key = ("small", E)
    if key not in _CACHE:
        rng = np.random.default_rng(1200 + E)
        sizes = [0, 1, 33 * E + 1, 1025 * E, 2050 * E + 1, TILE + 3 * E + 1, 3000, 16 * E, 1027 * E, 4099 * E, 2 * TILE, 7 * E]
        tensors = [rng.integers(0, 256, s, dtype=np.uint8) if k % 4 == 1 else np.concatenate([_walk(rng, s // E, E), np.zeros(s % E, np.uint8)]) for k, s in enumerate(sizes)]
        bases = []
        for k, t in enumerate(tensors):
            b = t.copy()
            if len(b):
                b[rng.integers(0, len(b), max(len(b) // 40, 1))] ^= 3
            bases.append(b if k % 3 else rng.integers(0, 256, len(t), dtype=np.uint8))
        _CACHE[key] = (tensors, bases)
    return _CACHE[key]


def _frames(dst, foff, first):
    dst, foff = dst.cpu().numpy(), foff.cpu().tolist()
    return [dst[foff[a]:foff[b]].tobytes() for a, b in zip(first, first[1:])]


@pytest.mark.parametrize("segment_log", [None, 10, 11])
@pytest.mark.parametrize("E", [2, 4])
def test_composites_given_and_chosen(hip, E, segment_log):
    tensors, bases = _small(E)
    n, S = len(tensors), pc.offsets(tensors)
    sizes = [len(t) for t in tensors]
    src, base = _dev(pc.cat(tensors)), _dev(pc.cat(bases))
    seg = segment_log is not None
    sf = hip.planes_segment_first(np.diff(S.astype(np.int64)), E, segment_log) if seg else None
    first = [int(sf[i * E]) for i in range(n + 1)] if seg else [i * E for i in range(n + 1)]

    def compress(tr, st, **kw):
        if seg:
            return hip.tensor_compress_seg_each_stride_dbatch(src, S, E, segment_log, tr, st, base, seg_first=sf, block_size_id=0, **kw)
        return hip.tensor_compress_each_stride_dbatch(src, S, E, tr, st, base, block_size_id=0, **kw)

    def decompress(frames, foff, tr, st, dst):
        if seg:
            return hip.tensor_decompress_seg_each_stride_dbatch(frames, foff, S, E, segment_log, tr, st, dst, sf, dst=dst)
        return hip.tensor_decompress_each_stride_dbatch(frames, foff, S, E, tr, st, dst, dst=dst)
    # the dedicated composites: the _pred_stride_ call of every stride, the _each_ composite for the transforms that have no stride
    ded = {}
    for s in pes.STRIDES:
        r = (hip.tensor_compress_seg_pred_stride_dbatch(src, S, E, s, segment_log, sf, block_size_id=0) if seg else hip.tensor_compress_pred_stride_dbatch(src, S, E, s, block_size_id=0))
        assert int(r[2].min()) >= 0
        ded[("S", s)] = _frames(r[0], r[1], first)
    for t in (PLAIN, XOR, SUB):
        r = (hip.tensor_compress_seg_each_dbatch(src, S, E, segment_log, [t] * n, base, seg_first=sf, block_size_id=0) if seg else
             hip.tensor_compress_each_dbatch(src, S, E, [t] * n, base, block_size_id=0))
        ded[t] = _frames(r[0], r[1], first)
    # GIVEN: the frames of the dedicated call of every tensor's transform and stride, and back in place over a copy of the bases
    for lead in (0, 31, 77):
        tr, st = pes.cycle_transforms_and_strides(n, lead)
        dst, foff, fres, tres, _, tro, sto = compress(tr, st)
        assert int(fres.min()) >= 0 and tres.cpu().tolist() == sizes and tro.cpu().tolist() == tr and sto.cpu().tolist() == st
        got = _frames(dst, foff, first)
        for i in range(n):
            assert got[i] == ded[("S", st[i]) if tr[i] == PRED else tr[i]][i], (E, segment_log, lead, i)
        held = base.clone()
        out, res = decompress(dst[:int(foff[-1])], foff, tr, st, held)
        assert res.cpu().tolist() == sizes and torch.equal(out, src)
    # a stride byte of 9 refuses its tensor alone, in the compress and in the decompress composite
    k = 4
    tr, st = list(tr), list(st)
    tr[k], st[k] = PRED, 3
    dst, foff, _, _, _, _, _ = compress(tr, st)
    bad = list(st)
    bad[k] = 9
    assert compress(tr, bad)[3].cpu().tolist() == [GENERIC if i == k else s for i, s in enumerate(sizes)]
    held = base.clone()
    out, res = decompress(dst[:int(foff[-1])], foff, tr, bad, held)
    a, b = int(S[k]), int(S[k + 1])
    assert res.cpu().tolist() == [GENERIC if i == k else s for i, s in enumerate(sizes)] and torch.equal(out[:a], src[:a]) and torch.equal(out[b:], src[b:])
    assert torch.equal(out[a:b], base[a:b]), "the refused tensor keeps its old bytes"
    # CHOOSE: the model's transforms and strides, and the frames GIVEN writes with them
    for mask, smask, margin, b in ((15, 0x0F, 50, bases), (3, 0xFF, 0, None), (2, 0x2A, 50, None), (15, 1, 50, bases)):
        want = pes.estimate_stride_model(tensors, E, mask, smask, b, margin)
        est = torch.full((n * 4 + 1,), -7, dtype=torch.int64, device="cuda")
        dst, foff, fres, tres, _, tro, sto = compress(None, None, candidate_mask=mask, stride_mask=smask, margin_permille=margin, est_bytes=est)
        assert tro.cpu().tolist() == want[2] and sto.cpu().tolist() == pes.settled(want[2], want[5]), (E, segment_log, mask, smask)
        assert [x & ONES for x in est.cpu().tolist()[:-1]] == want[1] and int(est[-1]) == -7
        assert int(fres.min()) >= 0 and tres.cpu().tolist() == sizes
        again = compress(tro, sto)
        assert torch.equal(again[1], foff) and torch.equal(again[0][:int(foff[-1])], dst[:int(foff[-1])]), "choose once, then give: the same frames"
        held = base.clone()
        out, res = decompress(dst[:int(foff[-1])], foff, tro, sto, held)
        assert res.cpu().tolist() == sizes and torch.equal(out, src)
        assert mask != 3 or len(set(sto.cpu().tolist())) >= 3, "the walks have several channel counts"
    # a damaged frame fails its tensor alone
    k = 4                                                       # 2050 elements and a byte: its first frame's last byte is the checksum's
    frames = dst[:int(foff[-1])].clone()
    frames[int(foff[first[k]]) + int(fres[first[k]]) - 1] ^= 0x40
    held = base.clone()
    out, res = decompress(frames, foff, tro, sto, held)
    res = res.cpu().tolist()
    a, b = int(S[k]), int(S[k + 1])
    assert res[k] < 0 and res[:k] + res[k + 1:] == sizes[:k] + sizes[k + 1:] and torch.equal(out[:a], src[:a]) and torch.equal(out[b:], src[b:]) and torch.equal(out[a:b], base[a:b])


def test_the_choosing_composite_in_a_hip_graph_follows_changed_sources(hip):
    import ctypes as C
    E, L, mask, smask = 2, 10, 3, 0x0F
    sizes = [3 * TILE + 4, 2052, TILE]
    n, cap = 3, sum(sizes)
    S = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    sf = hip.planes_segment_first(sizes, E, L)
    nf = int(sf[-1])
    blocks = hip.planes_block_bound(cap, n, E, 0)
    src, planes = (torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
    soff, sfd = _i64(S), _i64(sf)
    chosen, strides = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(hip.frame_packed_bound(cap, nf, blocks, 0), dtype=torch.uint8, device="cuda")
    foff, so = torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    fres, tres, poff = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (nf, n, n * E + 1))
    hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize.restype = C.c_size_t
    need = hip.tensor_each_stride_workspace_head(n, E, True, mask, smask) + int(hip.lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize(C.c_size_t(nf), C.c_size_t(blocks),
                                                                                                                                       C.c_uint(0), C.c_int(0)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def load(seed):
        rng = np.random.default_rng(seed)
        ts = [rng.integers(0, 256, s, dtype=np.uint8) if (k + seed) % 3 == 0 else _walk(rng, s // E + (seed + k) % 4, E)[:s] for k, s in enumerate(sizes)]
        src.copy_(_dev(pc.cat(ts)))
        return ts

    def work():
        hip.tensor_compress_seg_each_stride_dbatch(src, soff, E, L, None, None, None, mask, smask, 50, seg_first=sfd, n_segments=nf, block_size_id=0, dst=dst,
                                                   max_total_blocks=blocks, frame_offsets=foff, frame_results=fres, tensor_results=tres, planes=planes,
                                                   plane_offsets=poff, seg_offsets=so, workspace=ws, chosen=chosen, chosen_strides=strides)
    load(0)
    work()
    torch.cuda.synchronize()
    seen = [(chosen.cpu().tolist(), strides.cpu().tolist())]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    for seed in (1, 2):
        ts = load(seed)
        for t in (dst, foff, fres, tres, chosen, strides):
            t.fill_(3)
        ws.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        want = pes.estimate_stride_model(ts, E, mask, smask, None, 50)
        pair = (want[2], pes.settled(want[2], want[5]))
        assert (chosen.cpu().tolist(), strides.cpu().tolist()) == pair and pair not in seen, (seed, pair, seen)
        seen.append(pair)
        d, fo, _, _, _, _, _ = hip.tensor_compress_seg_each_stride_dbatch(_dev(pc.cat(ts)), S, E, L, pair[0], pair[1], seg_first=sf, block_size_id=0)
        assert foff.cpu().tolist() == fo.cpu().tolist() and torch.equal(dst[:int(foff[-1])], d[:int(fo[-1])]), seed
        out, res = hip.tensor_decompress_seg_each_stride_dbatch(dst[:int(foff[-1])], foff, S, E, L, pair[0], pair[1], seg_first=sf)
        assert res.cpu().tolist() == sizes and torch.equal(out, src)


# ---------------------------------------------------------------------------------------------------------------- Python
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("segment_log", [None, 16])
def test_compress_tensors_each_with_strides_on_a_mixed_list(hip, segment_log, tmp_path):
    from finitestateentropy_amd.api import CompressedTensors
    rows = pes.table(1 << 16)
    ts = [_dev(rows["stereo"][1]).view(torch.int16).reshape(-1, 2), _dev(rows["xyz"][1][:65535 * 4]).view(torch.float32).reshape(-1, 3),
          _dev(rows["boxes"][1]).view(torch.int32).reshape(-1, 4), _dev(rows["bf16_gaussian"][1]).view(torch.bfloat16), _dev(rows["sorted_int64"][1]).view(torch.int64)]
    keep = [t.clone() for t in ts]
    want_tr, want_st = ["pred", "pred", "pred", "plain", "pred"], [2, 3, 4, 1, 1]
    for E in (2, 4, 8):                                         # ... as the model says, group by group
        idx = [i for i, t in enumerate(ts) if t.element_size() == E]
        m = pes.estimate_stride_model([t.cpu().reshape(-1).view(torch.uint8).numpy() for t in (ts[i] for i in idx)], E, 3, 0x0F, None, 50)
        assert [pest.NAMES[c] for c in m[2]] == [want_tr[i] for i in idx] and pes.settled(m[2], m[5]) == [want_st[i] for i in idx]
    rec = hip.estimate_tensors(ts, strides=(1, 2, 3, 4))
    assert [r["choice"] for r in rec] == want_tr and [r["stride"] for r in rec][:3] == [2, 3, 4] and all(sorted(r["stride_estimates"]) == [1, 2, 3, 4] for r in rec)
    assert all(r["estimates"]["pred"] == r["stride_estimates"][r["stride"]] for r in rec)
    assert all(set(r) == {"bytes", "estimates", "choice"} for r in hip.estimate_tensors(ts)), "without strides the records are today's"
    obj = hip.compress_tensors_each(ts, "auto", strides=(1, 2, 3, 4), segment_log=segment_log)
    assert isinstance(obj, CompressedTensors) and obj.transforms == want_tr and obj.strides == want_st and obj.segment_log == segment_log
    plain = hip.compress_tensors_each(ts, "auto", segment_log=segment_log)
    assert plain.strides is None and plain.transforms[0] == "plain" and plain.transforms[4] == "pred" and obj.nbytes < plain.nbytes
    print("mixed list: stride 1 only %d frame bytes, strides chosen per tensor %d" % (plain.nbytes, obj.nbytes))
    again = hip.compress_tensors_each(ts, obj.transforms, strides=obj.strides, segment_log=segment_log)
    assert again.strides == obj.strides and all(torch.equal(a["frames"], b["frames"]) for a, b in zip(again.groups, obj.groups)), "choose once, then give"
    opened = hip.open_archive(hip.archive_tensors(obj))
    path = str(tmp_path / "mixed.fsa")
    hip.save_tensors(obj, path)
    loaded = hip.load_tensors(path)
    for o in (obj, opened, loaded):
        assert o.transforms == want_tr and o.strides == want_st and o.nbytes == obj.nbytes
        back = hip.decompress_tensors(o)
        for a, r, k in zip(ts, back, keep):
            assert a.dtype == r.dtype and a.shape == r.shape and _bits(a, r) and _bits(a, k)
    assert hip.open_archive(hip.archive_tensors(plain)).strides is None
    if segment_log is not None:
        for call in (lambda: hip.decompress_tensor_windows_each(obj, [None] * len(ts)), lambda: hip.patch_tensor_windows_each(obj, [None] * len(ts), [None] * len(ts))):
            with pytest.raises(ValueError, match="stride above 1"):
                call()
        assert hip.decompress_tensor_windows_each(plain, [(0, 5)] + [None] * 4)[0].numel() == 5, "stride 1 everywhere: windows as ever"
