"""The FSE decoder corpus (tests/fse_decode_corpus.py) on the CPU: the schedule model of k_fse_decode (scripts/sim/fse_decode_sim.py) reaches
every labelled hand-over, computes what the reference computes at every capacity the corpus uses, mirrors the kernel's constants, and is told
from every deliberately broken variant of its rules by at least one corpus block (mutation testing without running a faulty kernel).  The
device side is tests/test_gpu_fse_decode_paths.py."""
import os
import re
import time
from collections import Counter

import numpy as np
import pytest

import fse_decode_corpus as fc

dsim = fc.dsim
CSRC = os.path.join(fc.ROOT, "finitestateentropy_amd", "csrc")


@pytest.fixture(scope="module")
def corpus(checker):
    t0 = time.time()
    blocks, company = fc.build(checker)
    t1 = time.time()
    for b in blocks:
        fc.labels(b)                                    # (runs the model at the block's own capacities: cached in the block)
    print("\n  corpus: %d blocks built in %.2f s (of which the candidate search for the plain loop's rules: see SEARCH), "
          "modelled at their own capacities in %.2f s" % (len(blocks), t1 - t0, time.time() - t1))
    return blocks, company


def test_corpus_is_small(corpus):
    blocks, _ = corpus
    assert len(blocks) <= 400
    big = [b for b in blocks if b.n >= 32768]
    assert len(big) <= 6, [b.name for b in big]
    assert all(b.n < 4096 for b in blocks if b.n < 32768)
    assert len({b.name for b in blocks}) == len(blocks)


def test_every_label_is_reached(corpus):
    blocks, _ = corpus
    lab = Counter()
    c0 = set()
    for b in blocks:
        lab.update(fc.labels(b))
        for route in b.routes:
            c0.update(s["c0"] for s in (b.sim(cap, route) for cap in b.caps) if s["everBulk"])
    if len(c0) >= 8:
        lab["c0_variety"] = len(c0)
    print()
    for name in fc.LABELS:
        print("  %-26s %d" % (name, lab[name]))
    print("  chunk phases (c0) reached: %s" % sorted(c0))
    print("  plain-loop search: %s; r.at reached %s; q after the first phase reached %s" % (fc.SEARCH["found"], fc.SEARCH["at_reached"], fc.SEARCH["q_reached"]))
    for name, why in fc.UNREACHABLE.items():
        print("  not reachable: %s -- %s" % (name, why))
    missing = [k for k in fc.LABELS if not lab[k]]
    assert not missing, missing
    # values on both sides of each of the plain loop's rules
    at, q = fc.SEARCH["at_reached"], fc.SEARCH["q_reached"]
    assert any(v < 128 for v in at) and any(v >= 128 for v in at) and any(v < 124 for v in q) and any(v >= 124 for v in q)
    assert all(v % 4 == 0 for v in q)                   # (why there is no block at q == 123)


def test_model_equals_the_reference(corpus, checker):
    """result and bytes, every block, alone capacities and the capacities of the whole-corpus runs; on dstSize_tooSmall the bytes written
    up to there as well"""
    blocks, _ = corpus
    n = 0
    for b in blocks:
        for cap in sorted(set(b.caps) | set(fc.BATCH_CAPS)):
            s = b.sim(cap)
            r, out = checker.fse_decompress_using_dtable(b.payload, b.dt, cap)
            assert s["result"] == r, (b.name, cap, s["result"], r, s["nLong"], s["nFin"], s["handback"])
            k = r if r < (1 << 63) else min(len(s["out"]), cap)
            assert s["out"][:k] == out[:k].tobytes(), (b.name, cap)
            assert s["iters"] == 16 * s["nLong"] + 2 * s["nFin"] and (s["everBulk"] or s["iters"] == 0)
            n += 1
        if b.header is not None and not b.kind.startswith("damaged"):
            # the header carries the block's own table: the one-shot path decodes with the same cells
            h, msv, tl, norm = checker.fse_read_ncount(b.header)
            assert h == len(b.header)
            rr, dt = checker.fse_build_dtable(norm[:msv + 1], msv, tl)
            assert rr == 0 and np.array_equal(dt, b.dt), b.name
            r, out = checker.fse_decompress(b.oneshot_bytes(), b.n)
            assert r == b.n and (out[:r] == b.src).all(), b.name
    print("\n  model == reference on %d (block, capacity) pairs" % n)


def test_bad_tables_stay_inside_the_reference_contract(corpus):
    """what the issue allows of a table the staging pass refuses: newState not a multiple of 1 << nbBits, every reachable state inside the table,
    nbBits <= tableLog, an honest fast-mode flag"""
    blocks, _ = corpus
    bad = [b for b in blocks if b.kind == "bad"]
    assert len(bad) >= 4
    for b in bad:
        t = b.table
        ts = 1 << t.tl
        assert t.bad and all(ns + (1 << nb) <= ts and nb <= t.tl for ns, nb in zip(t.ns, t.nb)), b.name
        assert not (t.fast and t.nb0), b.name
        assert all(not b.sim(cap)["everBulk"] for cap in b.caps), b.name


def _define(text, name):
    m = re.search(r"^\s*#\s*define\s+%s\s+(\d+)u?\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_constants_mirror_the_sources():
    dec = open(os.path.join(CSRC, "fse_decode.hip")).read()
    internal = open(os.path.join(CSRC, "internal.h")).read()
    for name in ("FSE_CHECK_EVERY", "FSE_FINISH_EVERY", "FSE_DEC_RING", "FSE_IN_RING", "FSE_IN_CHUNK", "FSE_FLUSH_MIN", "FSE_DEC_WAVES"):
        assert getattr(dsim, name) == _define(dec, name), name
    for name in ("FSE_DBIN_LOG", "FSE_DEC_FAST_MAXLOG"):
        assert getattr(dsim, name) == _define(internal, name), name
    # the inequalities themselves, as the kernel writes them (a retune of the text leaves this test to be looked at, not silently behind)
    for text in ("Bstart >= 65 + 48 * (FSE_CHECK_EVERY - 1)", "Bstart >= 65 + 48 * (FSE_FINISH_EVERY - 1)", "r.at >= 24 + 6 * FSE_CHECK_EVERY + 8",
                 "bs.q >= 24u + 6u * FSE_CHECK_EVERY + 4u", "groups0 >= FSE_CHECK_EVERY", "groups0 >= FSE_FINISH_EVERY",
                 "Bp >= 65u + 48u * (FSE_CHECK_EVERY - 1)", "B - inA8 >= 65u + 48u * (FSE_FINISH_EVERY - 1)",
                 "if (it == NITER - 1) PheadRef = P;", "r.at = (size_t)((Bh + 7u) >> 3) - 8; r.used = 8u * ((u32)r.at + 8u) - B;"):
        assert text in dec, text


# Variants nothing in the result, the bytes, the phase counts or the rebuilt reader can catch, with the reason; none at present.
DECISION_ONLY = {}


def _pairs(blocks):
    """(block, capacity, route) from the cheapest up: a mutant is usually caught by a small block"""
    for b in sorted(blocks, key=lambda b: len(b.payload)):
        for route in b.routes:
            for cap in b.caps:
                yield b, cap, route


@pytest.mark.parametrize("mut", sorted(dsim.MUTANTS))
def test_corpus_catches_mutant(corpus, mut):
    blocks, _ = corpus
    for b, cap, route in _pairs(blocks):
        if b.n >= 32768:
            continue
        if dsim.view(b.sim(cap, route, mut=mut)) != dsim.view(b.sim(cap, route)):
            m, s = b.sim(cap, route, mut=mut), b.sim(cap, route)
            what = [k for k, x, y in zip(("nLong", "nFin", "reader", "result", "bytes"), dsim.view(m), dsim.view(s)) if x != y]
            print("\n  %s (%s): caught by %s, capacity %d, %s path: %s differ" % (mut, dsim.MUTANTS[mut], b.name, cap, route, ", ".join(what)))
            return
    if mut in DECISION_ONLY:
        print("\n  %s changes nothing observable: %s" % (mut, DECISION_ONLY[mut]))
        return
    pytest.fail("no corpus block tells the model from the mutant %s (%s)" % (mut, dsim.MUTANTS[mut]))


def test_company_and_bins(corpus):
    """the caller path's company workgroups: blocks that finish after 0, 1, 2, .. phases and damaged streams share a decoder wave with a 32 KB
    block; the one-shot path's size bins: populations that are no multiple of the workgroup's blocks, an empty bin between two occupied
    ones, the open-ended last bin occupied -- workgroups straddle bins"""
    blocks, company = corpus
    for name, (mtl, grp) in company.items():
        G = 33 if mtl <= dsim.FSE_DEC_FAST_MAXLOG else 18
        ppw = (G + dsim.FSE_DEC_WAVES - 1) // dsim.FSE_DEC_WAVES
        recs = [b.sim(fc.BATCH_CAPS[0]) for b in grp]
        for w in range(dsim.FSE_DEC_WAVES):
            mine = list(zip(grp, recs))[w * ppw:(w + 1) * ppw]
            if not any(b.n >= 32768 for b, _ in mine):
                continue
            phases = sorted({s["nLong"] + s["nFin"] for _, s in mine if s["loop"] == "rev"})
            assert len(phases) >= 5 and phases[0] == 0 and phases[-1] >= 300, (name, w, phases)
            assert sum(b.kind.startswith("damaged") for b, _ in mine) >= 3, (name, w)
    bins = fc.oneshot_bins(blocks)
    print()
    for cls, G in (("rev11", 33), ("rev12", 18), ("plain", 18)):
        pop = {k: len(v) for k, v in sorted(bins[cls].items())}
        print("  one-shot class %s (%d blocks a workgroup): bin populations %s" % (cls, G, pop))
    pop = {k: len(v) for k, v in bins["rev11"].items()}
    occupied = sorted(pop)
    assert 15 in occupied and len(occupied) >= 3
    assert any(b - a > 1 for a, b in zip(occupied, occupied[1:]))             # an empty bin between two occupied ones
    edges = np.cumsum([pop[k] for k in occupied])[:-1]
    assert all(e % 33 for e in edges), edges                                    # every bin boundary falls inside a workgroup


def test_corpus_is_deterministic(checker):
    a, _ = fc.build(checker)
    b, _ = fc.build(checker)
    assert [x.name for x in a] == [y.name for y in b]
    assert all(np.array_equal(x.payload, y.payload) and np.array_equal(x.dt, y.dt) for x, y in zip(a, b))
