"""The FSE decoder corpus (tests/fse_decode_corpus.py) through the device: every hand-over of k_fse_decode -- long phases, finishing phases,
the literal tail, the rebuilt reader -- against the compiled reference, result for result and byte for byte, through
FSE_decompress_usingDTable over a batch, FSE_decompress over a batch and the single-block host calls; every block alone, all of them in
corpus order and shuffled, on source rows of odd strides at every address modulo 4 (guard mode on: conftest.py); and the device's own phase
counters (the TIMED instantiation's g_decTiming, through FseHip.decode_timing) against the schedule model's (scripts/sim/fse_decode_sim.py):
    [2]  rounds that ran a long phase   == nLong of the model for a block alone; for a workgroup the sum over its decoder waves of the most
    [10] rounds of finishing phases     == nFin   any of the wave's blocks takes (rounds are wave-uniform, every chain that can run does) --
                                           as far as the wave's FIRST lane pair counts them: the counter a wave adds is lane 0's, and a pair
                                           whose block never enters the bulk stays out of the round loop (dsim.wave_rounds)
    [4]  += 1 by every decoder wave (FSE_DEC_WAVES a workgroup) of a TIMED workgroup that got as far as the bulk: a workgroup none of whose
         tables is the launch's returns before
The TIMED instantiation is a kernel of its own, so its results and bytes are asserted too.  The plain-cell loop (table log 12 with a cell of
nbBits 0) has no TIMED form: it is covered by results and bytes only -- on the caller path the TIMED launch before it must decline the block
and count no round.  On dstSize_tooSmall the bytes written up to there are compared as well (their number is the model's)."""
import numpy as np
import pytest
import torch

import fse_decode_corpus as fc
from oracle.oracle import err_code, is_error

pytestmark = pytest.mark.gpu
dsim = fc.dsim
G_OF = {11: 33, 12: 18}             # blocks per workgroup by LDS table log (fse_decode_geometry: 160 KB of LDS, 4 KiB / 8 KiB tables)


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.fixture(scope="module")
def corpus(checker):
    return fc.build(checker)


_REF = {}


def _ref(checker, b, cap, route):
    """computed once per (block, capacity, route) and shared by every test of the module"""
    key = (b.name, cap, route)
    if key not in _REF:
        if route == "caller":
            r, o = checker.fse_decompress_using_dtable(b.payload, b.dt, cap)
        else:
            r, o = checker.fse_decompress(b.oneshot_bytes(), cap)
        if is_error(r):
            k = min(len(b.sim(cap)["out"]), cap) if err_code(r) == 2 else 0
        else:
            k = r
        _REF[key] = (s64(r), o[:k].copy())
    return _REF[key]


def _check(checker, items, res, out, route, cap, what):
    for i, b in enumerate(items):
        r, o = _ref(checker, b, cap, route)
        assert res[i] == r, (what, route, b.name, cap, i, int(res[i]), r)
        assert (out[i][:len(o)] == o).all(), (what, route, b.name, cap, i)


def _run(hip, items, cap, route, mtl=12, pad=13, off=0):
    """-> (results, bytes, payload addresses modulo 64)"""
    if route == "caller":
        csrc, sizes, addrs = fc.device_rows(torch, [b.payload for b in items], pad, off)
        out, res = hip.fse_decompress_using_dtable_batch(csrc, sizes, fc.device_tables(torch, items, mtl), cap, max_table_log=mtl)
    else:
        csrc, sizes, addrs = fc.device_rows(torch, [b.oneshot_bytes() for b in items], pad, off)
        out, res = hip.fse_decompress_batch(csrc, sizes, cap, max_log=12)
    return res.cpu().numpy(), out.cpu().numpy(), addrs


def _mtl(b, i):
    return 12 if b.table.tl == 12 or i % 2 == 0 else 11


@pytest.mark.parametrize("route", ["caller", "oneshot"])
def test_every_block_alone(hip, checker, corpus, route):
    """nBlocks = 1, every capacity of the block, the row at the block's own address"""
    blocks, _ = corpus
    n = 0
    for i, b in enumerate(blocks):
        if route not in b.routes:
            continue
        for cap in b.caps:
            res, out, addrs = _run(hip, [b], cap, route, _mtl(b, i), pad=1 + 2 * (i % 7), off=b.off)
            assert addrs[0] == b.off
            _check(checker, [b], res, out, route, cap, "alone")
            n += 1
    print("\n  %s path: %d single-block decodes" % (route, n))


@pytest.mark.parametrize("route", ["caller", "oneshot"])
def test_all_together_and_shuffled(hip, checker, corpus, route):
    """the whole corpus in one call: corpus order (the caller path keeps it: slot g of a workgroup is block first + g) and shuffled, with
    everything fitting and with 16 groups of room; row strides odd, the first row at an odd address"""
    blocks, _ = corpus
    items = [b for b in blocks if route in b.routes]
    orders = [list(range(len(items))), list(np.random.RandomState(11).permutation(len(items)))]
    for k, order in enumerate(orders):
        its = [items[j] for j in order]
        for cap in fc.BATCH_CAPS:
            res, out, _ = _run(hip, its, cap, route, 12, pad=7 + 2 * k, off=3 + 18 * k)
            _check(checker, its, res, out, route, cap, "together" if k == 0 else "shuffled")


def test_single_block_host_calls(hip, checker, corpus):
    """a sample through FSE_decompress_usingDTable / FSE_decompress on host pointers.  These calls hand the destination back only when the
    result is a size (the bytes of a failed call stay in device memory), so on an error the result alone is compared"""
    blocks, _ = corpus
    for b in blocks[::5] + [x for x in blocks if x.kind == "bad"]:
        cap = b.caps[-1]
        r, o = hip.fse_decompress_using_dtable(b.payload, b.dt, cap)
        er, eo = _ref(checker, b, cap, "caller")
        assert s64(r) == er and (er < 0 or (o[:er] == eo[:er]).all()), (b.name, cap, r, er)
        if b.header is not None:
            r, o = hip.fse_decompress(b.oneshot_bytes(), cap)
            er, eo = _ref(checker, b, cap, "oneshot")
            assert s64(r) == er and (er < 0 or (o[:er] == eo[:er]).all()), (b.name, cap, r, er)


@pytest.mark.parametrize("route", ["caller", "oneshot"])
def test_phase_counters_alone(hip, checker, corpus, route):
    """every block alone through the TIMED kernel: long and finishing rounds equal the model's phase counts (a table the staging pass
    refuses, and one the launch declines, count none); results and bytes are the reference's"""
    blocks, _ = corpus
    n, top = 0, (0, 0)
    for i, b in enumerate(blocks):
        if route not in b.routes:
            continue
        rev = b.loop == "rev"
        for cap in b.caps:
            with hip.decode_timing() as t:
                res, out, addrs = _run(hip, [b], cap, route, _mtl(b, i), pad=1 + 2 * (i % 7), off=b.off)
            _check(checker, [b], res, out, route, cap, "timed")
            s = b.sim(cap, route)
            want = (s["nLong"], s["nFin"]) if rev else (0, 0)
            waves = dsim.FSE_DEC_WAVES if rev or route == "caller" else 0      # (the one-shot PLAIN class has no TIMED launch at all)
            assert (t[2], t[10], t[4]) == (want[0], want[1], waves), (route, b.name, cap, t[2], t[10], t[4], want, s["decisions"][:3])
            n += 1
            top = max(top, want)
    print("\n  %s path: model == device on %d single-block decodes; most rounds (long, finishing): %s" % (route, n, top))


def _expect_rounds(items, addrs, cap, mtl):
    """(long rounds, finishing rounds, decoder waves) the caller path's TIMED launches add for a batch in order: the 4 KiB class over all
    blocks (slots of table-log-12 blocks empty), then -- maxTableLog 12 -- the 8 KiB class (slots of the others empty; tables with a cell
    of nbBits 0 declined)"""
    recs = [b.sim(cap, "caller", row_addr=a) for b, a in zip(items, addrs)]
    total = [0, 0, 0]
    for lds_log in ((11, 12) if mtl == 12 else (11,)):
        G = G_OF[lds_log]
        mine = [(b.table.tl == 12) == (lds_log == 12) for b in items]
        slots = [r if m and b.loop == "rev" else None for b, r, m in zip(items, recs, mine)]
        for w in range(0, len(items), G):
            if any(mine[w:w + G]):
                total[0] += dsim.wave_rounds(slots[w:w + G], G, "nLong")
                total[1] += dsim.wave_rounds(slots[w:w + G], G, "nFin")
                total[2] += dsim.FSE_DEC_WAVES
    return tuple(total)


def test_phase_counters_in_company(hip, checker, corpus):
    """workgroups of the caller path in which blocks that finish after 0, 1, 2, .. phases, damaged streams among them, ride along with a
    32 KB block; two workgroups in one launch; and the whole corpus in order"""
    blocks, company = corpus
    cap = fc.BATCH_CAPS[0]
    groups = [(name, mtl, grp) for name, (mtl, grp) in company.items()]
    groups.append(("wg11_a+b", 11, company["wg11_a"][1] + company["wg11_b"][1]))
    groups.append(("corpus", 12, blocks))
    for name, mtl, grp in groups:
        with hip.decode_timing() as t:
            res, out, addrs = _run(hip, grp, cap, "caller", mtl, pad=9, off=21)
        _check(checker, grp, res, out, "caller", cap, name)
        want = _expect_rounds(grp, addrs, cap, mtl)
        print("\n  %s: long rounds %d, finishing rounds %d, decoder waves %d (model: %s)" % (name, t[2], t[10], t[4], want))
        assert (t[2], t[10], t[4]) == want, (name, t[2], t[10], t[4], want)
    # the quirk named in the module docstring is really in play: wave 1 of wg11_b runs rounds that its first lane pair does not count
    a = _expect_rounds(company["wg11_a"][1], [0] * 33, cap, 11)
    b = _expect_rounds(company["wg11_b"][1], [0] * 33, cap, 11)
    assert a[0] > b[0] > 0
