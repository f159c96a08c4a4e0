"""Double-symbol (X2) tables on the stream-parallel Huff0 decoder, on the CPU: the restatement of the kernel's derivation (derive_x2 in
scripts/sim/huf_par_sim.py, huf_decode_par.hip:347-421) accepts every table the compiled reference builds and derives the reference's own
single-symbol table from it; the corpus of tests/huf_x2_par_corpus.py reaches every label, every damaged table is declined by the rule it was
aimed at while the reference's outcome is not the block, and the corpus tells every deliberately broken variant of the model from the model
(mutation testing without running a faulty kernel).  The device side is tests/test_gpu_huf_x2_par.py.

How a dropped rule shows.  Four rules guard symbols and bit counts that only the double-symbol decoder reads (len1_bits, len2_bits, nbtot_le_log,
second_follows): without the rule the derivation vouches, the walk returns (dst_size, block) and the reference returns something else -- the
mutant is caught by bytes or result AGAINST THE REFERENCE.  The others cannot show that way:
  runs, pow2_aligned   a table that breaks only one of these is one both decoders read alike (a cell relabelled with another symbol of the same
                       length: each decodes that code as the other symbol), so what the mutant returns is the reference's answer; the
                       single-cell damages of these rules also break a bit-count rule behind them.  Caught by the decision (`parallel`).
  n_lt_ts, len_1_or_2  only the constant table and a length field of 0 or 3 break them, and those stay off the device and, for the lengths, away
                       from the reference (its loops advance by the field).  Caught by the decision; without n < ts the model reports the hang.
  second_present       implied by len2_bits: an absent symbol counts 255 bits, and no byte equals n1 + 255 with n1 >= 1.  No input tells a
                       derivation without it from the kernel's; asserted as such below."""
from collections import Counter

import numpy as np
import pytest

import huf_x2_corpus as xc
import huf_x2_par_corpus as pc
from oracle.oracle import is_error

hsim = pc.hsim
BY_BYTES = ("len1_bits", "len2_bits", "nbtot_le_log", "second_follows")
BY_DECISION = ("runs", "pow2_aligned", "n_lt_ts", "len_1_or_2")
IMPLIED = ("second_present",)
X2_MUTANTS = sorted(m for m in hsim.MUTANTS if m.startswith("x2_"))


@pytest.fixture(scope="module")
def corpus(ref, restatement):
    """[(entry, the model's record at max_table_log 12, the reference's (result, bytes))] -- built once, never changed"""
    out = []
    for e in pc.build(ref, restatement):
        r, o = (None, None) if e.name in ("len_0", "len_3") else e.reference(ref)
        out.append((e, e.simulate(), (r, o)))
    return out


def test_reference_built_tables_are_accepted(ref, restatement):
    """every table HUF_readDTableX2 builds from the headers of tests/huf_x2_corpus.py is accepted, and the derived cells {first symbol, its
    length} are HUF_readDTableX1's table for the same header, expanded to the double-symbol table's log"""
    n, logs = 0, set()
    for name, hdr, L in xc.build(ref, restatement):
        r, dt = ref.huf_read_dtable_x2(hdr, L)
        if is_error(r):
            continue
        acc, clause, cells = hsim.derive_x2(dt)
        assert acc, (name, clause)
        r1, d1 = ref.huf_read_dtable_x1(hdr, 11)
        assert r1 == r, name
        tl = (int(d1[0]) >> 16) & 0xFF
        x1 = d1[1:1 + ((1 << tl) + 1) // 2].view(np.uint16)[:1 << tl].astype(np.int64)
        assert (cells == x1[np.arange(1 << L) >> (L - tl)]).all(), name
        n += 1
        logs.add(L)                                                      # (the table's log is the limit it was read at)
    assert n == 159, n
    assert logs >= set(range(1, 13)), logs


def test_every_label_is_reached(corpus):
    lab = Counter()
    for e, rec, _ in corpus:
        lab.update(pc.labels(e, rec, e.simulate(decode=False, max_table_log=11)))
    print()
    for name in pc.LABELS:
        print("  %-24s %d" % (name, lab[name]))
    assert set(lab) <= set(pc.LABELS), set(lab) - set(pc.LABELS)
    assert not [k for k in pc.LABELS if not lab[k]]
    assert len(corpus) <= 150 and all(len(e.blk) <= 65536 for e, _, _ in corpus)


def test_damaged_tables_are_declined_by_their_rule(corpus):
    """... and, for every one of them, the reference's outcome is not (dst_size, block): a kernel that vouched would be seen"""
    per = Counter()
    for e, rec, (r, o) in corpus:
        if e.kind == "benign":
            assert hsim.derive_x2(e.dt)[0] and rec["parallel"], e.name
        if e.clause is None:
            continue
        assert hsim.derive_x2(e.dt)[:2] == (False, e.clause), (e.name, hsim.derive_x2(e.dt)[:2])
        assert rec["reason"] == "table" and not rec["entered"], e.name
        per[e.clause] += 1
        if e.kind == "damaged_table":
            assert not e.cpu_only
            assert r != e.dst_size or not np.array_equal(o[:r], e.blk), e.name
            assert set((e.dt[1:1 + (1 << e.table_log)] >> 24).tolist()) <= {1, 2}, e.name
        else:
            assert e.cpu_only, e.name
    assert set(per) == set(pc.CLAUSES), per
    print("\n  declined per rule:", dict(per))


def test_parallel_blocks_regenerate_the_reference(corpus):
    n_par, logs = 0, set()
    for e, rec, (r, o) in corpus:
        if rec["parallel"]:
            assert r == e.dst_size and (rec["out"] == o[:r]).all(), e.name
            n_par += 1
            logs.add(e.table_log)
    assert n_par >= 40 and logs >= set(range(1, 13)), (n_par, logs)


def _view(rec):
    return (rec["parallel"], rec["entered"], rec["rounds"], rec["bad"], None if rec["out"] is None else rec["out"].tobytes())


@pytest.mark.parametrize("mut", X2_MUTANTS)
def test_corpus_catches_x2_mutant(corpus, mut):
    rule = mut[6:] if mut.startswith("x2_no_") else None
    seen = []
    for e, rec, (r, o) in corpus:
        if rule and e.clause is None:
            continue                                                     # (a dropped rule changes nothing for a table that keeps every rule)
        m = e.simulate(mut=mut)
        if rule in BY_BYTES:
            if m["parallel"] and (r != e.dst_size or not np.array_equal(o[:r], m["out"])):
                assert np.array_equal(m["out"], e.blk) or e.name.endswith("_badpl"), e.name      # it vouched: the valid payload gives the block
                seen.append(e.name)
        elif rule in BY_DECISION:
            if (m["parallel"], m["entered"]) != (rec["parallel"], rec["entered"]):
                seen.append(e.name)
        elif _view(m) != _view(rec):
            seen.append(e.name)
    print("\n  %s (%s): %s" % (mut, hsim.MUTANTS[mut], "told by %d entries, first %s" % (len(seen), seen[0]) if seen else "told by none"))
    if rule in IMPLIED:
        assert not seen, seen                                            # (see the module's docstring: if this changes, the rule has become observable)
    else:
        assert seen, "no corpus entry tells the model from the mutant %s (%s)" % (mut, hsim.MUTANTS[mut])


def test_single_symbol_blocks_ignore_the_x2_mutants(checker):
    """the X2 variants leave the walk of a single-symbol table alone (tests/repair_corpus.py's blocks keep their records)"""
    import repair_corpus as rc
    for e in rc.huf_entries(checker)[:6]:
        rec = e.simulate(decode=False)
        for mut in ("x2_small_pieces", "x2_len_from_cell", "x2_no_runs"):
            assert _view(e.simulate(mut=mut, decode=False)) == _view(rec), (e.name, mut)


def test_without_accept_x2_the_block_is_declined(corpus):
    """the 4X1 / 1X1 entry points and the one-shot path never take a double-symbol table: reason "block", as before"""
    e = corpus[0][0]
    for kw in (dict(), dict(accept_x2=True, oneshot=True)):
        rec = hsim.simulate_block(e.payload, e.dt, e.dst_size, e.form, **kw)
        assert rec["reason"] in ("block", "prep") and not rec["entered"], kw


def test_corpus_is_deterministic(corpus, ref, restatement):
    again = pc.build(ref, restatement)
    assert [e.name for e in again] == [e.name for e, _, _ in corpus]
    for a, (b, _, _) in zip(again, corpus):
        assert a.payload.tobytes() == b.payload.tobytes() and a.dt.tobytes() == b.dt.tobytes() and a.dst_size == b.dst_size and a.labels == b.labels, a.name
