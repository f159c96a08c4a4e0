"""The bit-reversed loop's rounds in which EVERY chain of a decoder wave runs (k_fse_decode, csrc/fse_decode.hip: the loop entered on
`__all(can)`), and the hand-over between that loop and the rounds that carry zombies.  Streams are built with the fixed-cost tables of
tests/fse_decode_corpus.py, so every value a round decides on is hit exactly; every result and every byte is compared with the reference,
and the device's phase counters (the TIMED instantiation, FseHip.decode_timing: [2] long rounds, [10] finishing rounds, [4] decoder waves)
with the schedule model's (scripts/sim/fse_decode_sim.py).

What the loop does differently from the round with zombies, and which test lands on it:
  * `can` after a phase is ONE unsigned compare of max(Bp - 785, grp - 16): 785 / 784 bits and 16 / 15 groups left after 1 .. 5 rounds inside
    the loop (test_long_rule_inside_the_loop), and the values twice as far out -- 65 + 48*31 = 1553 / 1552 bits, 32 / 31 groups -- that a
    round head would have to decide on before it could take two phases in one round (test_values_two_phases_out);
  * the ring position is iters modulo the ring size, and `rpos` / `q` of the other rounds are rebuilt when the loop ends: blocks that leave
    the loop at ring positions 16, 32, 48 and 0, before and after the ring has wrapped, and go on with finishing phases (test_ring_positions);
  * both lanes of a pair store the control words; the poll is one compare of a minimum: a workgroup of 33 equal blocks, which stays in the
    loop from its first round to its last long phase (test_uniform_workgroup);
  * one block of a workgroup of 33 ends 1, 2 and 17 phases before the others, in either decoder wave: the loop hands over to the round with
    zombies, which finishes the others (test_mixed_wave);
  * the same at table log 12 (8 KiB slots, 18 blocks a workgroup) and through FSE_decompress_usingDTable with maxTableLog 11
    (the `klass` parameter of the workgroup tests)."""
import numpy as np
import pytest
import torch

import fse_decode_corpus as fc
from oracle.oracle import err_code, is_error

pytestmark = pytest.mark.gpu
dsim = fc.dsim
PER_PHASE = 4 * dsim.FSE_CHECK_EVERY           # symbols a long phase decodes
# table class -> (bits per symbol of the raw table, maxTableLog of the call, blocks per workgroup)
KLASS = {"log11": (5, 11, 33), "log12": (12, 12, 18)}


def raw_block(orc, name, nb, n, off=0, seed=1):
    """fc.raw_block with a destination of two bytes per symbol: FSE_compressBound covers 8 bits per symbol and the raw table of table log
    12 writes 12"""
    _, ct = orc.fse_build_ctable_raw(nb)
    _, dt = orc.fse_build_dtable_raw(nb)
    src = fc._rs(nb, n, seed).randint(0, min(256, 1 << nb), n).astype(np.uint8)
    r, out = orc.fse_compress_using_ctable(src, ct, cap=2 * n + 64)
    assert 0 < r <= 2 * n + 64, (name, r)
    return fc.Block(name, out[:r], dt, n, None, None, off, "raw%d" % nb, src)


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


_REF = {}


def _ref(checker, b, cap):
    """the reference's result and bytes, computed once per (block, capacity) and shared by every test of the module"""
    key = (b.name, cap)
    if key not in _REF:
        r, o = checker.fse_decompress_using_dtable(b.payload, b.dt, cap)
        k = (min(len(b.sim(cap)["out"]), cap) if err_code(r) == 2 else 0) if is_error(r) else r
        _REF[key] = (s64(r), o[:k].copy())
    return _REF[key]


def _decode(hip, checker, items, cap, mtl, what, pad=9, off=5):
    """the batch through the TIMED kernel of the caller path, results and bytes checked -> (counters, row addresses modulo 64)"""
    csrc, sizes, addrs = fc.device_rows(torch, [b.payload for b in items], pad, off)
    with hip.decode_timing() as t:
        out, res = hip.fse_decompress_using_dtable_batch(csrc, sizes, fc.device_tables(torch, items, mtl), cap, max_table_log=mtl)
    res, out = res.cpu().numpy(), out.cpu().numpy()
    for i, b in enumerate(items):
        r, o = _ref(checker, b, cap)
        assert res[i] == r, (what, b.name, cap, i, int(res[i]), r)
        assert (out[i][:len(o)] == o).all(), (what, b.name, cap, i)
    # ... and through the product's own instantiation (no counters): the same bytes
    out2, res2 = hip.fse_decompress_using_dtable_batch(csrc, sizes, fc.device_tables(torch, items, mtl), cap, max_table_log=mtl)
    assert (res2.cpu().numpy() == res).all() and (out2.cpu().numpy() == out).all(), (what, cap)
    return t, addrs


def _alone(hip, checker, b, cap, mtl, what):
    t, addrs = _decode(hip, checker, [b], cap, mtl, what, pad=3, off=b.off)
    s = b.sim(cap, "caller", row_addr=addrs[0])
    assert (t[2], t[10], t[4]) == (s["nLong"], s["nFin"], dsim.FSE_DEC_WAVES), (what, b.name, cap, t[2], t[10], s["nLong"], s["nFin"])
    return s


def _workgroup(hip, checker, items, cap, mtl, G, what):
    assert len(items) == G
    t, addrs = _decode(hip, checker, items, cap, mtl, what)
    recs = [b.sim(cap, "caller", row_addr=a) for b, a in zip(items, addrs)]
    want = (dsim.wave_rounds(recs, G, "nLong"), dsim.wave_rounds(recs, G, "nFin"), dsim.FSE_DEC_WAVES)
    assert (t[2], t[10], t[4]) == want, (what, t[2], t[10], t[4], want)
    return recs


def test_long_rule_inside_the_loop(hip, checker):
    """one bit per symbol: a block of n symbols has n - 2 bits unread at the start and 64 fewer after every long phase"""
    for k in range(1, 6):
        for bits, long_next in ((785, True), (784, False)):
            b = raw_block(checker, "r1_after%d_%d" % (k, bits), 1, bits + 2 + 64 * k, off=(7 * k + bits) & 63)
            s = _alone(hip, checker, b, b.n, 11, "bits")
            d = s["decisions"][k]
            assert (d["kind"], d["B"], d["long"]) == ("after_long", bits, long_next) and s["nLong"] == k + long_next
    big = raw_block(checker, "r1_roomy", 1, 4000, off=11)                  # plenty of bits: the groups decide
    for k in range(1, 6):
        for g, long_next in ((16, True), (15, False)):
            cap = 4 * (16 * k + g) + (0 if long_next else 3)
            s = _alone(hip, checker, big, cap, 11, "groups")
            d = s["decisions"][k]
            assert (d["kind"], d["groups"], d["long"]) == ("after_long", g, long_next) and d["B"] >= 785 and s["nLong"] == k + long_next


def test_values_two_phases_out(hip, checker):
    """65 + 48 * 31 bits and one fewer, 32 groups and one fewer, at a round head after 0 .. 4 rounds: where two phases in a row stop being
    certain -- a round that took both on such a value would show in the long-phase count or in the bytes"""
    edge = 65 + 48 * (2 * dsim.FSE_CHECK_EVERY - 1)
    for k in range(0, 5):
        for bits in (edge, edge - 1):
            b = raw_block(checker, "r1_head%d_%d" % (k, bits), 1, bits + 2 + 64 * k, off=(5 * k + bits) & 63)
            s = _alone(hip, checker, b, b.n, 11, "bits x2")
            assert s["decisions"][k]["B"] == bits and s["nLong"] == k + (bits - 785) // 64 + 1
    big = raw_block(checker, "r1_roomy", 1, 4000, off=11)
    for k in range(0, 5):
        for g in (32, 31):
            s = _alone(hip, checker, big, 4 * (16 * k + g) + (g & 1), 11, "groups x2")
            assert s["decisions"][k]["groups"] == g and s["nLong"] == k + g // 16


@pytest.mark.parametrize("klass", sorted(KLASS))
def test_ring_positions(hip, checker, klass):
    """blocks that leave the loop after 1 .. 9 long phases: ring positions 16, 32, 48, 0 and, wrapped, 16 .. 48, 0, 16 -- the finishing
    phases that follow write at the rebuilt position, the service wave reads there"""
    nb, mtl, _ = KLASS[klass]
    for k in range(1, 10):
        # k long phases, then finishing phases down to < 113 bits: 785 - 48 * 15 = 65 bits short of another long phase at the most
        n = PER_PHASE * k + (65 + 48 * 15) // nb - 20
        b = raw_block(checker, "r%d_pos%d" % (nb, k), nb, n, off=(3 * k) & 63, seed=k)
        s = _alone(hip, checker, b, b.n, mtl, "ring position")
        assert s["nLong"] == k and s["nFin"] >= 1


@pytest.mark.parametrize("klass", sorted(KLASS))
def test_uniform_workgroup(hip, checker, klass):
    """a full workgroup of equal blocks (other bytes in each): both decoder waves stay in the loop from the first round to the last long one"""
    nb, mtl, G = KLASS[klass]
    items = [raw_block(checker, "r%d_uni%d" % (nb, g), nb, PER_PHASE * 21 + 50, seed=100 + g) for g in range(G)]
    recs = _workgroup(hip, checker, items, items[0].n, mtl, G, "uniform " + klass)
    assert all(r["nLong"] == recs[0]["nLong"] >= 20 for r in recs)


@pytest.mark.parametrize("klass", sorted(KLASS))
@pytest.mark.parametrize("early", [1, 2, 17])
def test_mixed_wave(hip, checker, klass, early):
    """one block ends `early` long phases before the 32 (17) others, once in each decoder wave and never in a wave's first slot (whose
    counters the wave reports): the loop hands the wave over to the rounds with zombies, which take the others to their end"""
    nb, mtl, G = KLASS[klass]
    long_n = PER_PHASE * 24 + 50
    ppw = (G + dsim.FSE_DEC_WAVES - 1) // dsim.FSE_DEC_WAVES
    for slot in (3, ppw + 5):
        items = [raw_block(checker, "r%d_mix%d" % (nb, g), nb, long_n, seed=200 + g) for g in range(G)]
        items[slot] = raw_block(checker, "r%d_mix_short%d" % (nb, early), nb, long_n - PER_PHASE * early, seed=300 + early)
        recs = _workgroup(hip, checker, items, long_n, mtl, G, "mixed %s slot %d" % (klass, slot))
        assert recs[0]["nLong"] - recs[slot]["nLong"] == early and recs[slot]["nLong"] >= 1
