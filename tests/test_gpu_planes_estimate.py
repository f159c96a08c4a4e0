"""Plane estimates on the device (FSEHIP_planes_estimate_dbatch and the Python surface around estimate_tensors / compress_tensors_auto) against
the integer model of planes_estimate_corpus.py -- np.bincount over the planes that the split models write, the header's cost arithmetic --
with exact equality of all four outputs; never against the library's own calls.  Outputs are pre-filled with -7 and have a spare entry
behind them that must stay -7; sources and bases carry 0xA5 tails and must come back unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_corpus as pc
import planes_estimate_corpus as pe
import planes_pred_corpus as ppc
import planes_sub_corpus as psc
from planes_corpus import GENERIC, TILE
from planes_estimate_corpus import NAMES, NO_CHOICE, ONES

pytestmark = pytest.mark.gpu

FILL, TAIL, MARK = 0xA5, 64, 0xF9                            # MARK: -7 as a choice byte
SHIFTS = ((0, 0), (1, 5), (8, 15), (3, 2))                  # source and base, each off 16-byte alignment by an amount of its own
HIP_INVALID_VALUE = 1
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _filled(n, shift=0, content=None):
    t = torch.full((shift + n + TAIL,), FILL, dtype=torch.uint8, device="cuda")[shift:]
    if content is not None and len(content):
        t[:len(content)] = _dev(content)
    return t


def counts(E):
    """the element counts of the issue"""
    per = TILE // E
    return [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, per - 1, per, per + 1, 3 * per + 5]


def across(E, stride):
    """every ordered pair of edge values as neighbours across a boundary (the construction of test_gpu_planes_pred.py): pair k lies at the
    elements stride (k + 1) - 1 | stride (k + 1), on a smooth ramp.  stride 1024: run boundaries"""
    vals = ppc.edge_values(E)
    pairs = [(x, y) for x in vals for y in vals]
    seq = (np.arange(stride * (len(pairs) + 1) + 3, dtype=np.uint64) * np.uint64(3)) & np.uint64((1 << (8 * E - 1)) - 1 if E < 8 else (1 << 40) - 1)
    for k, (x, y) in enumerate(pairs):
        seq[stride * (k + 1) - 1], seq[stride * (k + 1)] = x, y
    return seq.astype(ppc._U[E]).view(np.uint8).copy()


def _near(t, rng):
    """a base for t: t with one byte in ten changed"""
    b = t.copy()
    hit = rng.random(len(b)) < 0.1
    b[hit] ^= rng.integers(1, 256, int(hit.sum()), dtype=np.uint8)
    return b


def _corpus(E):
    """-> (tensors, bases): every count of the issue as whole elements and again with n mod E != 0; sixty tensors of 0 .. 40 bytes that share
    a tile; a smooth tensor of more than five tiles; all zeros and all 0xFF over three tiles and 5 bytes (the hot bin and its partial last
    chunk); tensor == base; the edge values as neighbours, across run boundaries, and as (tensor, base) pairs.  The bases: the tensor with
    a tenth of its bytes changed, or random bytes, alternating"""
    if E not in _CACHE:
        rng = np.random.default_rng(900 + E)
        tensors, bases = [], []

        def add(t, b=None):
            t = np.ascontiguousarray(t, np.uint8)
            tensors.append(t)
            bases.append(np.ascontiguousarray(b, np.uint8) if b is not None else _near(t, rng) if len(tensors) % 2 else rng.integers(0, 256, len(t), dtype=np.uint8))
        for k, c in enumerate(counts(E)):
            add(rng.integers(0, 256, c * E, dtype=np.uint8))
            add(rng.integers(0, 256, c * E + (1 + k % (E - 1) if E > 1 else 0), dtype=np.uint8))
        tiny = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(0, 41, 60)]
        assert sum(len(t) for t in tiny) < TILE // 8
        for t in tiny:
            add(t)
        steps = rng.integers(-3, 4, 5 * TILE // E + 77).astype(np.int64)
        smooth = np.concatenate([(np.cumsum(steps) + 1000).astype(np.uint64).astype(ppc._U[E]).view(np.uint8), np.arange(1, E, dtype=np.uint8)])
        add(smooth, _near(smooth, rng))
        zeros, ffs = np.zeros(3 * TILE + 5, np.uint8), np.full(3 * TILE + 5, 0xFF, np.uint8)
        nearly = zeros.copy()
        nearly[[7, TILE + 1, 3 * TILE + 4]] = (1, 0x80, 0xFF)
        add(zeros, nearly)
        add(ffs, ffs)
        same = rng.integers(0, 256, 2 * TILE + 3, dtype=np.uint8)
        add(same, same)
        add(ppc.edge_sequence(E, 15))
        add(across(E, 1024))
        t, b = psc.edge_pairs(E, 3)
        add(t, b)
        add(b, t)
        _CACHE[E] = (tensors, bases)
    return _CACHE[E]


def _model(E):
    """the model of the whole corpus with every candidate, margin 50 -- computed once and shared"""
    key = ("model", E)
    if key not in _CACHE:
        tensors, bases = _corpus(E)
        _CACHE[key] = pe.estimate_model(tensors, E, 15, bases, 50)
    return _CACHE[key]


def masked(full, E, mask, margin, refused=()):
    """what the call returns for `mask` and `margin`, from the model of all four candidates: the slots of candidates outside the mask are
    all-ones, the choice is the rule's over the others; the tensors in `refused` are refused"""
    bits, est, _, res = full
    n = len(res)
    b, e, ch, r = [], [], [], []
    for i in range(n):
        if i in refused:
            b += [ONES] * (4 * E); e += [ONES] * 4; ch.append(NO_CHOICE); r.append(GENERIC)
            continue
        for c in range(4):
            on = (mask >> c) & 1
            b += bits[(i * 4 + c) * E:(i * 4 + c + 1) * E] if on else [ONES] * E
            e.append(est[i * 4 + c] if on else ONES)
        ch.append(pe.choose(e[-4:], mask, margin))
        r.append(res[i])
    return b, e, ch, r


def run_estimate(hip, tensors, bases, E, mask=15, margin=50, capacity=None, shift=(0, 0), offsets=None):
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
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    hip.planes_estimate_dbatch(src[:total], S, E, mask, margin, base=None if base is None else base[:total], capacity=capacity, plane_bits=pb, est_bytes=eb,
                               choice=ch, results=res)
    torch.cuda.synchronize()
    assert int(pb[-1]) == -7 and int(eb[-1]) == -7 and int(ch[-1]) == MARK and int(res[-1]) == -7, "the entry behind every output"
    host = src.cpu().numpy()
    assert (host[:total] == flat).all() and (host[total:] == FILL).all(), "the source is only read"
    if base is not None:
        host = base.cpu().numpy()
        assert (host[:total] == bflat).all() and (host[total:] == FILL).all(), "the base is only read"
    return ([x & ONES for x in pb.cpu().tolist()[:-1]], [x & ONES for x in eb.cpu().tolist()[:-1]], ch.cpu().tolist()[:-1], res.cpu().tolist()[:-1])


def check(got, want, what):
    for name, g, w in zip(("plane bits", "estimates", "choice", "results"), got, want):
        assert len(g) == len(w), (what, name)
        bad = [k for k in range(len(w)) if g[k] != w[k]]
        assert not bad, (what, name, bad[:8], [g[k] for k in bad[:4]], [w[k] for k in bad[:4]])


# ---------------------------------------------------------------------------------------------------------------- the C call
@pytest.mark.parametrize("E", pc.ELEMS)
def test_estimate_against_the_model(hip, E):
    tensors, bases = _corpus(E)
    sizes = [len(t) for t in tensors]
    assert all(c * E in sizes for c in counts(E)) and (E == 1 or all(any(c * E < s < (c + 1) * E for s in sizes) for c in counts(E)))
    assert sum(1 for s in sizes if s <= 40) >= 60 and max(sizes) > 5 * TILE and sizes.count(3 * TILE + 5) >= 2
    full = _model(E)
    same = [i for i, (t, b) in enumerate(zip(tensors, bases)) if len(t) > TILE and (t == b).all()]
    assert len(same) >= 2 and all(full[1][4 * i + 2] == full[1][4 * i + 3] == 0 for i in same), "tensor == base: the delta planes are all zeros, the estimates 0"
    zeros = next(i for i, t in enumerate(tensors) if len(t) == 3 * TILE + 5 and not t.any())
    assert full[1][4 * zeros] == full[1][4 * zeros + 1] == 0 and 0 < full[1][4 * zeros + 2] < 64
    for shift in SHIFTS:
        check(run_estimate(hip, tensors, bases, E, shift=shift), full, (E, shift))


@pytest.mark.parametrize("E", pc.ELEMS)
def test_every_mask_and_margin(hip, E):
    tensors, bases = _corpus(E)
    full = _model(E)
    for mask in range(1, 16):
        margin = (0, 50, 1000)[mask % 3]
        check(run_estimate(hip, tensors, bases, E, mask, margin, shift=SHIFTS[mask % 4]), masked(full, E, mask, margin), (E, mask, margin))
    for mask in (1, 2, 3):                                     # without a base
        check(run_estimate(hip, tensors, None, E, mask, 50, shift=SHIFTS[mask]), masked(full, E, mask, 50), (E, mask, "no base"))
    for margin in (0, 50, 1000):
        got = run_estimate(hip, tensors, bases, E, 15, margin, shift=SHIFTS[1])
        check(got, masked(full, E, 15, margin), (E, margin))
    assert len({tuple(masked(full, E, 15, m)[2]) for m in (0, 50, 1000)}) == 3, "the three margins choose differently on this corpus"
    assert set(masked(full, E, 15, 1000)[2]) == {0}, "margin 1000: the lowest requested id everywhere"


@pytest.mark.parametrize("E", pc.ELEMS)
def test_estimate_with_a_short_capacity(hip, E):
    tensors, bases = _corpus(E)
    full = _model(E)
    S = [int(x) for x in pc.offsets(tensors)]
    k = next(i for i, t in enumerate(tensors) if len(t) == TILE)
    for cap in (S[k] + 100, S[k + 1], S[k + 1] - 1, S[6], 0):  # inside a tensor, at a tensor's end, one short of it, at an early end, nothing
        refused = {i for i in range(len(tensors)) if S[i + 1] > cap}
        assert refused and (cap == 0 or len(refused) < len(tensors))
        got = run_estimate(hip, tensors, bases, E, capacity=cap, shift=SHIFTS[1])
        check(got, masked(full, E, 15, 50, refused), (E, cap))
        assert pe.estimate_model(tensors[:8], E, 15, bases[:8], 50, capacity=cap)[3] == got[3][:8], "the model's own refusals"


@pytest.mark.parametrize("E", pc.ELEMS)
def test_estimate_refuses_a_decreasing_slot(hip, E):
    rng = np.random.default_rng(43)
    flat, bflat = rng.integers(0, 256, 320, dtype=np.uint8), rng.integers(0, 256, 320, dtype=np.uint8)
    offsets = [0, 100, 60, 200, 300, 370]                       # slot 1 decreases, slot 4 ends behind the capacity
    units = [flat[a:b] if a <= b <= 320 else flat[:0] for a, b in zip(offsets, offsets[1:])]
    bunits = [bflat[a:b] if a <= b <= 320 else bflat[:0] for a, b in zip(offsets, offsets[1:])]
    want = pe.estimate_model(units, E, 15, bunits, 50, capacity=320, offsets=offsets)
    assert want[3] == [100, GENERIC, 140, 100, GENERIC] and want[2][1] == want[2][4] == NO_CHOICE
    got = run_estimate(hip, [flat], [bflat], E, capacity=320, offsets=offsets)
    check(got, want, E)
    assert got[1][4:8] == [ONES] * 4 and got[0][4 * E:8 * E] == [ONES] * (4 * E)


def test_argument_errors_write_nothing(hip):
    E, n = 2, 3
    src, base = _filled(300), _filled(300)
    soff = torch.tensor([0, 100, 200, 300], dtype=torch.int64, device="cuda")
    pb = torch.full((n * 4 * E + 1,), -7, dtype=torch.int64, device="cuda")
    eb = torch.full((n * 4 + 1,), -7, dtype=torch.int64, device="cuda")
    ch = torch.full((n + 1,), MARK, dtype=torch.uint8, device="cuda")
    res = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    need = hip.planes_estimate_workspace_bound(n, E, 15)
    ws = torch.full((need + 256,), FILL, dtype=torch.uint8, device="cuda")
    VP, SZ, UI, U64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_uint64
    good = dict(pb=pb.data_ptr(), eb=eb.data_ptr(), ch=ch.data_ptr(), res=res.data_ptr(), src=src.data_ptr(), base=base.data_ptr(), soff=soff.data_ptr(), n=n, E=E, cap=300,
                mask=15, margin=50, ws=ws.data_ptr(), wb=need)

    def call(**kw):
        a = dict(good, **kw)
        return hip.lib.FSEHIP_planes_estimate_dbatch(VP(a["pb"]), VP(a["eb"]), VP(a["ch"]), VP(a["res"]), VP(a["src"]), VP(a["base"]), VP(a["soff"]), SZ(a["n"]), UI(a["E"]),
                                                     U64(a["cap"]), UI(a["mask"]), UI(a["margin"]), VP(a["ws"]), SZ(a["wb"]), VP(torch.cuda.current_stream().cuda_stream))
    bad = [dict(pb=0), dict(eb=0), dict(ch=0), dict(res=0), dict(src=0), dict(soff=0), dict(mask=0), dict(mask=16), dict(mask=0x8000000F), dict(base=0),
           dict(base=0, mask=4), dict(base=0, mask=9), dict(E=0), dict(E=3), dict(E=16), dict(margin=1001), dict(wb=need - 1), dict(ws=0), dict(ws=ws.data_ptr() + 8),
           dict(n=1 << 24), dict(cap=1 << 46)]
    for kw in bad:
        assert call(**kw) == HIP_INVALID_VALUE, kw
    torch.cuda.synchronize()
    assert bool((pb == -7).all()) and bool((eb == -7).all()) and bool((ch == MARK).all()) and bool((res == -7).all()) and bool((ws == FILL).all()), "nothing is written"
    assert call(base=0, mask=3) == 0, "no base is needed for PLAIN and PRED"
    assert call(n=0) == 0, "no tensors: legal"
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [100, 100, 100, -7] and ch.cpu().tolist()[:3] != [MARK] * 3 and int(ch[3]) == MARK


def test_estimate_in_a_hip_graph_replayed_over_changed_sources(hip):
    """the call captured into a graph -- launches only, the counters zeroed by a launch of its own -- and replayed twice over changed source
    bytes: each replay gives the model of what the source held at that time, nothing is left over from the replay before"""
    E, mask, margin = 2, 15, 50
    sizes = [0, 3 * TILE + 5, 777, TILE, 2 * TILE + 3]
    n, S = len(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(S[-1])

    def pair(seed):
        rng = np.random.default_rng(seed)
        ts = [pc.bf16_gaussian((s + 1) // 2, seed=seed + k)[:s] if k % 2 else rng.integers(0, 4, s, dtype=np.uint8) for k, s in enumerate(sizes)]
        return ts, [_near(t, rng) for t in ts]
    src, base = torch.zeros(total, dtype=torch.uint8, device="cuda"), torch.zeros(total, dtype=torch.uint8, device="cuda")
    soff = torch.from_numpy(S.astype(np.int64)).cuda()
    pb = torch.zeros(n * 4 * E, dtype=torch.int64, device="cuda")
    eb, res = torch.zeros(n * 4, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    ch = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hip.planes_estimate_workspace_bound(n, E, mask), dtype=torch.uint8, device="cuda")

    def work():
        hip.planes_estimate_dbatch(src, soff, E, mask, margin, base=base, plane_bits=pb, est_bytes=eb, choice=ch, results=res, workspace=ws)

    def load(seed):
        ts, bs = pair(seed)
        src.copy_(_dev(pc.cat(ts))); base.copy_(_dev(pc.cat(bs)))
        return pe.estimate_model(ts, E, mask, bs, margin)

    def outputs():
        torch.cuda.synchronize()
        return [x & ONES for x in pb.cpu().tolist()], [x & ONES for x in eb.cpu().tolist()], ch.cpu().tolist(), res.cpu().tolist()
    want = load(0); work()                                      # one ordinary call first
    check(outputs(), want, "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    seen = [want]
    for seed in (100, 200):
        want = load(seed)
        assert want[1] not in [w[1] for w in seen]
        seen.append(want)
        for t in (pb, eb, res, ch):
            t.fill_(3)
        ws.fill_(0x5A)                                         # whatever the workspace holds: the call zeroes what it counts into
        g.replay()
        check(outputs(), want, ("replay", seed))


# ---------------------------------------------------------------------------------------------------------------- Python
def _bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _named():
    """the corpora of the header's table as CUDA tensors: name -> (tensor, base or None, the transform the estimate must choose)"""
    if "named" not in _CACHE:
        t, b = pe.update_pair()
        _CACHE["named"] = {
            "bf16 gaussian": (_dev(pe.bf16_gaussian()).view(torch.bfloat16), None, "plain"),
            "sorted int64": (_dev(pe.sorted_int64()).view(torch.int64), None, "pred"),
            "position ids": (_dev(pe.position_ids()).view(torch.int32).reshape(8, 4096), None, "pred"),
            "bf16 update": (_dev(t).view(torch.bfloat16), _dev(b).view(torch.bfloat16), "sub")}
    return _CACHE["named"]


TABLE = {"bf16 gaussian": dict(plain=174431, pred=183556), "sorted int64": dict(plain=163731, pred=108410), "position ids": dict(plain=49152, pred=108),
         "bf16 update": dict(plain=174431, pred=183556, xor=33297, sub=28881)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_estimate_tensors_chooses_what_really_is_smallest(hip, name):
    from finitestateentropy_amd.api import DeltaBase, PredictedPlanes
    t, b, want = _named()[name]
    (rec,) = hip.estimate_tensors([t], base=None if b is None else [b])
    assert rec == dict(bytes=t.numel() * t.element_size(), estimates=TABLE[name], choice=want), "the header's table row, and the choice"
    real = {"plain": hip.compress_tensors([t]).nbytes, "pred": hip.compress_tensors([t], PredictedPlanes(0)).nbytes}
    if b is not None:
        real["xor"] = hip.compress_tensors([t], base=[b]).nbytes
        real["sub"] = hip.compress_tensors([t], base=DeltaBase([b], "sub")).nbytes
    print("%-14s estimates %s, frame bytes %s" % (name, rec["estimates"], real))
    assert sorted(real) == sorted(rec["estimates"]) and min(real, key=real.get) == want and all(real[want] < v for k, v in real.items() if k != want)


@pytest.mark.parametrize("segment_log", [None, 18])
def test_compress_tensors_auto_on_a_mixed_list(hip, segment_log):
    from finitestateentropy_amd.api import TensorBundle
    named = _named()
    rng = np.random.default_rng(5)
    order = ("sorted int64", "bf16 gaussian", "bf16 update", "position ids")
    ts = [named[k][0] for k in order] + [torch.zeros((0, 7), dtype=torch.float32, device="cuda"), _dev(rng.integers(0, 256, 5005, dtype=np.uint8)).reshape(5, 1001)]
    # the bases of the whole list: the update's own, and for every other tensor something unrelated of its dtype and shape
    bases = [_dev(rng.integers(0, 1 << 40, 1 << 15).astype("<u8").view(np.uint8)).view(torch.int64), _dev(pc.bf16_gaussian(1 << 17, seed=9)).view(torch.bfloat16),
             named["bf16 update"][1], _dev(rng.integers(0, 1 << 30, 1 << 15).astype("<u4").view(np.uint8)).view(torch.int32).reshape(8, 4096),
             torch.zeros((0, 7), dtype=torch.float32, device="cuda"), _dev(rng.integers(0, 256, 5005, dtype=np.uint8)).reshape(5, 1001)]
    keep = [t.clone() for t in ts]
    for base in (None, bases):
        bundle = hip.compress_tensors_auto(ts, base=base, segment_log=segment_log)
        assert isinstance(bundle, TensorBundle) and set(bundle.parts) == set(bundle.index) <= set(NAMES)
        assert sorted(i for idx in bundle.index.values() for i in idx) == list(range(len(ts))), "every position in exactly one part"
        choices = [r["choice"] for r in bundle.estimates]
        assert choices == ["pred", "plain", "sub" if base is not None else "plain", "pred", "pred", "plain"], "the tensor of no bytes goes with the other 4-byte one"
        assert all(bundle.index[name] == [i for i, c in enumerate(choices) if c == name] for name in bundle.parts)
        assert [r["bytes"] for r in bundle.estimates] == [t.numel() * t.element_size() for t in ts]
        assert all(sorted(r["estimates"]) == sorted(NAMES if base is not None else NAMES[:2]) for r in bundle.estimates)
        for name, part in bundle.parts.items():
            assert part.segment_log == segment_log and part.delta == (name in ("xor", "sub")) and (part.predictor == "prev") == (name == "pred")
            assert name != "sub" or part.delta_op == "sub"
        assert bundle.nbytes == sum(p.nbytes for p in bundle.parts.values()) > 0
        back = hip.decompress_tensors(bundle, base=base)
        assert len(back) == len(ts)
        for a, r, k in zip(ts, back, keep):
            assert a.dtype == r.dtype and a.shape == r.shape and a.device == r.device and _bits(a, r) and _bits(a, k)
        if base is not None:
            assert "sub" in bundle.parts
            with pytest.raises(ValueError):
                hip.decompress_tensors(bundle)
            with pytest.raises(ValueError):
                hip.decompress_tensors(bundle, base=bases[:-1])
        else:
            plain = hip.compress_tensors(ts)
            print("mixed list, %d bytes: plain planes %d frame bytes, chosen per tensor %d" % (sum(r["bytes"] for r in bundle.estimates), plain.nbytes, bundle.nbytes))
            assert bundle.nbytes < plain.nbytes
