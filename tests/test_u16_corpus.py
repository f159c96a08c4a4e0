"""The corpus of the 16-bit-symbol coder (tests/u16_corpus.py) on the CPU: the route model (scripts/sim/u16_codec_sim.py) reaches every label,
computes what the compiled reference computes -- results, compressed bytes, regenerated symbols, the symbols written in front of an error --
at every capacity the corpus uses, mirrors the kernels' constants, and is told from each listed broken rule set by at least one block
(mutation testing without running a faulty kernel).  The device side is tests/test_gpu_u16_paths.py.  Skips as a whole without the compiled
reference."""
import os
import re
import time

import numpy as np
import pytest

import u16_corpus as uc

sim = uc.sim
CSRC = os.path.join(uc.ROOT, "finitestateentropy_amd", "csrc")
BATCH_CAPS = uc.BATCH_CAPS


@pytest.fixture(scope="module")
def corpus(ref):
    t0 = time.time()
    D, C = uc.build(ref)
    t1 = time.time()
    lab = uc.corpus_labels(D, C)
    print("\n  corpus: %d decode and %d compress blocks built in %.2f s, modelled at their own capacities in %.2f s" % (len(D), len(C), t1 - t0, time.time() - t1))
    return D, C, lab


def test_corpus_is_small(corpus):
    D, C, _ = corpus
    assert len(D) <= 300 and len(C) <= 200
    assert all(b.n <= 20000 for b in D + C)
    assert sum(b.n <= 2100 for b in D) * 10 >= len(D) * 8 and sum(b.n <= 4200 for b in C) * 10 >= len(C) * 9        # most blocks are small
    assert len({b.name for b in D}) == len(D) and len({b.name for b in C}) == len(C)


def test_every_label_is_reached(corpus):
    D, C, lab = corpus
    print()
    for name in uc.LABELS:
        print("  %-44s %s" % (name, "reached" if name in lab else "MISSING"))
    for name, why in uc.UNREACHABLE.items():
        print("  not reachable: %s -- %s" % (name, why))
    print("  searches: %s" % uc.SEARCH)
    missing = [k for k in uc.LABELS if k not in lab]
    assert not missing, missing
    assert not set(uc.UNREACHABLE) & set(uc.LABELS)
    assert len(set(uc.LABELS)) == len(uc.LABELS)
    stray = sorted(k for k in lab if k not in uc.LABELS)
    assert not stray, stray                              # every label the model can give is listed
    # a slowly mixing table needs at least two repair rounds
    assert max(b.sim(b.bound)["rounds"] or 0 for b in C if b.name.startswith("slow")) >= 2
    # the blocks kept from the search for a lane of exactly 8 bits stay with the wave kernel
    assert all(b.sim(b.bound)["route"] == "wave" and "c:lane_with_exactly_8_bits" in b.sim(b.bound)["labels"] for b in C if b.kind == "eight")


def test_fixed_cost_tables_hold_the_bits_they_claim(corpus):
    """B after the state read, which the model derives from the bytes, is the sum of the symbols' costs"""
    D, _, _ = corpus
    k = 0
    for b in D:
        if b.bits is not None:
            s = b.sim(b.n)
            assert s["B0"] == b.bits, (b.name, s["B0"], b.bits)
            k += 1
    assert k >= 60


def test_decode_model_equals_the_reference(corpus, ref):
    """result and symbols, every block, its own capacities and those of the whole-corpus runs; in front of an error the symbols written up to
    there as well (the model's count of them is what the device must have written)"""
    D, _, _ = corpus
    n = 0
    for b in D:
        for cap in sorted(set(b.caps) | set(BATCH_CAPS)):
            s = b.sim(cap)
            assert len(s["out"]) <= cap
            assert s["iters"] == 16 * s["nLong"] + s["nFin"]
            if not b.defined:
                assert s["result"] == uc.ferr("srcSize_wrong")                   # (documented device behaviour, include/fsehip.h)
                continue
            r, out = ref.fse_decompress_u16(b.comp, cap)
            assert s["result"] == r, (b.name, cap, s["result"], r, s["nLong"], s["nFin"], s["handover"])
            if not uc.is_err(r):
                assert len(s["out"]) == r
            assert s["out"] == out[:len(s["out"])].tolist(), (b.name, cap)
            if not uc.is_err(r) and b.src is not None and cap >= b.n:
                assert r == b.n and (out[:r] == b.src).all(), b.name
            n += 1
    print("\n  decode model == reference on %d (block, capacity) pairs" % n)


def test_compress_model_equals_the_reference(corpus, ref):
    """result and bytes at every capacity; where the reference is undefined (8 bytes or less behind a header that fits) the model gives the
    header writer's verdict, which IS defined: checked against FSE_writeNCount"""
    _, C, _ = corpus
    n = u = 0
    for b in C:
        for cap in b.caps:
            s = b.sim(cap)
            if b.ref_defined(cap):
                r, out = ref.fse_compress_u16(b.src, b.msv, b.tl, cap=cap)
                assert s["result"] == r, (b.name, cap, s["result"], r)
                if not uc.is_err(r) and r > 1:
                    assert s["out"][:r] == out[:r].tobytes(), (b.name, cap)
                n += 1
            else:
                f = b.facts
                r, out = ref.fse_write_ncount(cap, f["norm"], f["msv"], f["tl"])
                assert s["result"] == r, (b.name, cap, s["result"], r)
                u += 1
    print("\n  compress model == reference on %d (block, capacity) pairs; %d more where only the header writer is defined" % (n, u))
    assert n >= 150 and u >= 8


def test_ncount_writer_equals_the_reference(corpus, ref):
    """the writer that makes the hand-made headers: the reference's bytes wherever the reference's writer applies (table logs up to 12), its
    verdicts at every capacity around a header's size, and a read-back through FSE_readNCount everywhere"""
    D, C, _ = corpus
    seen = set()
    for b in D:
        if b.parsed is None or uc.is_err(b.parsed[0]) or b.kind.startswith("damaged"):
            continue
        h, msv, tl, norm = b.parsed
        key = (tl, norm[:msv + 1].tobytes())
        if key in seen:
            continue
        seen.add(key)
        mine = uc._write_ncount(norm[:msv + 1], msv, tl)
        assert bytes(mine) == bytes(b.comp[:h]), b.name
        if tl <= 12:
            r, out = ref.fse_write_ncount(600, norm[:msv + 1], msv, tl)
            assert r == len(mine) and bytes(out[:r]) == bytes(mine), b.name
            for cap in sorted({0, 1, 2, 3, h // 2, h - 3, h - 2, h - 1, h, h + 1, h + 2}):
                if cap < 0:
                    continue
                r, out = ref.fse_write_ncount(cap, norm[:msv + 1], msv, tl)
                v = uc._write_ncount(norm[:msv + 1], msv, tl, cap)
                assert (r == v) if isinstance(v, int) else (r == len(v) and bytes(out[:r]) == bytes(v)), (b.name, cap, r)
    assert len(seen) >= 20
    assert any(k[0] == 13 for k in seen)


def test_header_sizes_the_boundaries_rest_on(ref):
    """flat headers of 16 / 36 / 85 / 198 bytes, twelve-bit tables of 355 / 396, two-symbol blocks of 2,048 and 4,096 symbols with a 2-byte
    header at a requested table log of 5 and a 3-byte one at the default (what the `word in front of the row` bail-out needs)"""
    assert [uc.flat_block(ref, "f", k, 50).parsed[0] for k in (5, 6, 7, 8)] == [16, 36, 85, 198]
    assert [uc.nb12_block(ref, "t", 50, used=u).parsed[0] for u in (256, 286)] == [355, 396]
    for n in (2048, 4096):
        assert [len(uc.CBlock(ref, "two", uc.u16_data("two", n, 1), tl=tl).facts["header"]) for tl in (5, 0)] == [2, 3]


def test_damaged_streams_mostly_stay_defined(corpus):
    D, _, _ = corpus
    st = uc.DAMAGE_STATS
    print("\n  damaged streams: %d generated, %d kept (the reference is defined)" % (st["generated"], st["kept"]))
    assert st["generated"] >= 100 and st["kept"] * 10 >= st["generated"] * 9
    kept = [b for b in D if b.kind.startswith("damaged_")]
    assert len(kept) == st["kept"] and all(b.defined for b in kept)
    assert all(sum(b.kind == "damaged_" + how for b in kept) >= 10 for how in uc.DAMAGE)


def _define(text, name):
    m = re.search(r"^\s*#\s*define\s+%s\s+\(?(\d+)u?\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_constants_mirror_the_sources():
    enc = open(os.path.join(CSRC, "fse_u16.hip")).read()
    dec = open(os.path.join(CSRC, "fse_u16_decode.hip")).read()
    for name in ("U16_WAVE_MIN", "U16_LINE"):
        assert getattr(sim, name) == _define(enc, name), name
    for name in ("U16D_PHASE", "U16D_RING", "U16D_IN_RING", "U16D_IN_MIRROR", "U16D_IN_CHUNK", "U16D_FLUSH_MIN"):
        assert getattr(sim, name) == _define(dec, name), name
    assert "#define U16D_LDS (160 * 1024)" in dec and "#define U16_RING (2u * U16_LINE)" in enc
    # the rules themselves, as the kernels write them (a retune of the text leaves this test to be looked at, not silently behind)
    for text in ("B0 >= 65 + 48 * U16D_PHASE && grp >= U16D_PHASE", "B0 >= 65 + 48 && grp >= 1", "(Bp >= 65u + 48u * U16D_PHASE) & (grp >= U16D_PHASE)",
                 "(Bp >= 65u + 48u) & (grp >= 1)", "S < (1ull << 28)", "r.at = (size_t)((B + 7u) >> 3) - 8; r.used = 8u * ((u32)r.at + 8u) - B;",
                 "iters + U16D_PHASE - fl <= U16D_RING"):
        assert text in dec, text
    for text in ("n64 < U16_WAVE_MIN", "(u32)top1 * 64u > (63u << tl)", "mine && bits < 8u", "((blockDst + m.hdrSize) & ~(uintptr_t)3) < blockDst",
                 "cap > 8 && (size_t)(total >> 3) < cap - 8", "sum >= (n64 - 1) * 2", "if (i + 192 < nvec)", "warm < 64u ? 64u : (warm > 2048u ? 2048u : warm)"):
        assert text in enc, text
    assert 65 + 48 * sim.U16D_PHASE == 833 and 65 + 48 == 113
    assert sim.launch_geometry(11) == 33 and sim.launch_geometry(12) == 18


@pytest.mark.parametrize("mut", sorted(sim.MUTANTS))
def test_corpus_catches_mutant(corpus, mut):
    """each broken rule set changes the labels, the phase counts, the hand-over or the result of at least one block"""
    D, C, _ = corpus
    if mut in ("long_832", "fin_112", "groups_gt_16"):
        for b in sorted(D, key=lambda b: len(b.comp)):
            for cap in b.caps:
                if sim.view(b.sim(cap, mut=mut)) != sim.view(b.sim(cap)):
                    print("\n  %s (%s): caught by %s at capacity %d" % (mut, sim.MUTANTS[mut], b.name, cap))
                    return
    else:
        for b in sorted(C, key=lambda b: b.n):
            for cap in b.caps:
                m, s = b.sim(cap, mut=mut), b.sim(cap)
                if (m["labels"], m["result"], m["route"]) != (s["labels"], s["result"], s["route"]):
                    print("\n  %s (%s): caught by %s: %s" % (mut, sim.MUTANTS[mut], b.name, sorted(m["labels"] ^ s["labels"])))
                    return
    pytest.fail("no corpus block tells the model from the mutant %s (%s)" % (mut, sim.MUTANTS[mut]))


def test_workgroups_of_mixed_fate(corpus):
    """what tests/test_gpu_u16_paths.py relies on: each company is exactly one workgroup's range of its launch and holds every kind of
    neighbour at once"""
    D, _, _ = corpus
    cap = BATCH_CAPS[0]
    for name, (cls, grp) in uc.decode_company(D).items():
        G = sim.launch_geometry(cls)
        assert len(grp) == G, (name, len(grp), G)
        recs = [b.sim(cap) for b in grp]
        mine = [s["cls"] == cls for s in recs]
        lab = set().union(*(s["labels"] for s in recs))
        assert {"d:header_error", "d:nothing_behind_header", "d:builder_tl_13", "d:tablelog_above_13"} <= lab, (name, lab)
        assert any(s["cls"] == (12 if cls == 11 else 11) for s in recs), name
        assert any(m and not s["everBulk"] for m, s in zip(mine, recs)), name
        assert sum(m and b.n >= 18000 for m, b in zip(mine, grp)) == 1 and sum(m and b.n < 200 for m, b in zip(mine, grp)) >= 6, name
        assert any(not any(mine[g:g + 4]) for g in range(0, G, 4)), name          # a service wave with none of the launch's blocks
        phases = sorted({s["nLong"] for m, s in zip(mine, recs) if m})
        assert phases[0] == 0 and phases[-1] >= 100, (name, phases)


def test_corpus_is_deterministic(ref):
    a, c = uc.build(ref)
    b, d = uc.build(ref)
    assert [x.name for x in a] == [y.name for y in b] and [x.name for x in c] == [y.name for y in d]
    assert all(np.array_equal(x.comp, y.comp) for x, y in zip(a, b)) and all(np.array_equal(x.src, y.src) for x, y in zip(c, d))
