"""Double-symbol (X2) tables through the stream-parallel Huff0 decoder (k_huf_decode_par<HPAR_DATA_LARGE, true>, csrc/huf_decode_par.hip) on the
device: the corpus of tests/huf_x2_par_corpus.py against the compiled reference block by block, through the dispatching and the strict batch
calls at max_table_log 12 and 11, alone, among blocks with single-symbol tables and behind one shared table; and the model
(scripts/sim/huf_par_sim.py: derive_x2 and the walk with the X2 launch's piece size) against the device's own record of the HPAR_STATS build --
which blocks entered the parallel path, their repair rounds and bad links.  The CPU side is tests/test_huf_x2_par_model.py."""
from collections import Counter

import numpy as np
import pytest
import torch

import huf_x2_par_corpus as pc
import repair_corpus as rc
from oracle.oracle import is_error
from test_gpu_repair_paths import _child, s64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(ref, restatement):
    """[(entry, {max_table_log: the reference's (result, bytes)})] of the device entries -- computed once, never changed"""
    return [(e, {L: e.reference(ref, L) for L in (12, 11)}) for e in pc.build(ref, restatement) if not e.cpu_only]


def _check(items, res, out, L=12):
    for i, (e, want) in enumerate(items):
        r, exp = want[L]
        assert res[i] == s64(r), (e.name, L, res[i], s64(r))
        if not is_error(r):
            assert (out[i][:r] == exp[:r]).all(), (e.name, L)


def _fns(hip, form):
    return (hip.huf_decompress1x_using_dtable_batch, hip.huf_decompress1x2_using_dtable_batch) if form == 1 else \
           (hip.huf_decompress4x_using_dtable_batch, hip.huf_decompress4x2_using_dtable_batch)


@pytest.mark.parametrize("form", [4, 1])
def test_x2_model_matches_device(corpus, tmp_path, form):
    """HPAR_STATS build, one batched HUF_decompress4X / 1X_usingDTable call in a child process: a block left a record exactly when the model
    says it entered the parallel path (table accepted, block regular); there the repair rounds and bad links are the model's; results and
    bytes are the reference's; and for every table log 1 .. 12 some block entered and finished parallel (nothing passes by declining all)"""
    items = [it for it in corpus if it[0].form == form]
    assert len(items) <= 4096
    d = _child("hparstats", "x2_%d" % form, tmp_path)
    rec, res = d["rec"], d["res"]
    entered, declined, n_cmp = Counter(), Counter(), 0
    for i, (e, _) in enumerate(items):
        sim = e.simulate(decode=False)
        assert (rec[i, 2] != 0) == sim["entered"], (e.name, rec[i, :3], sim["entered"], sim["reason"], sim.get("clause"))
        if sim["entered"]:
            assert (int(rec[i, 0]), int(rec[i, 1])) == (sim["rounds"], sim["bad"]), (e.name, rec[i, :2], sim["rounds"], sim["bad"])
            n_cmp += 1
            if sim["parallel"] and res[i] == e.dst_size:
                entered[e.table_log] += 1
        elif sim["reason"] == "table":
            declined[sim["clause"]] += 1
    _check(items, res, d["out"])
    print("\n  Huff0 %dX, double-symbol tables: model == device on %d blocks; entered and finished parallel per table log: %s; "
          "declined per rule: %s" % (form, n_cmp, dict(sorted(entered.items())), dict(declined)))
    assert all(entered[t] for t in range(1, 13)), entered


@pytest.mark.parametrize("form", [4, 1])
def test_product_batches_against_reference(hip, corpus, form):
    """the whole device corpus through the dispatching and the strict batch call at max_table_log 12 and 11 (the 4 KiB table slot; a table of
    log 12 is then tableLog_tooLarge): the reference's result codes and bytes, block by block, the binding's guard bytes on"""
    assert hip.guard
    items = [it for it in corpus if it[0].form == form]
    c, cs, dt, ds = rc.huf_device_batch([e for e, _ in items], torch)
    for L in (12, 11):
        assert any(e.table_log > L for e, _ in items) == (L == 11)
        for fn in _fns(hip, form):
            out, res = fn(c, cs, dt, ds, max_table_log=L)
            _check(items, res.cpu().numpy(), out.cpu().numpy(), L)


@pytest.mark.parametrize("form", [4, 1])
def test_batch_independence(hip, ref, checker, corpus, form):
    """every entry alone, and all of them shuffled among blocks with single-symbol tables (tests/repair_corpus.py: parallel, repaired, handed
    over, serial-only): the lean launch, the X2 launch and the literal kernels leave one another's blocks alone"""
    items = [it for it in corpus if it[0].form == form]
    fn = _fns(hip, form)[0]
    x1 = [e for e in rc.huf_entries(checker) if e.form == form]
    dec = ref.huf_decompress1x_using_dtable if form == 1 else ref.huf_decompress4x_using_dtable
    pool = items + [(e, {12: dec(e.payload, e.dt, e.dst_size)}) for e in x1]
    assert len(x1) >= 10
    rng = np.random.RandomState(11 + form)
    mix = [pool[k] for k in rng.permutation(len(pool))]
    c, cs, dt, ds = rc.huf_device_batch([e for e, _ in mix], torch)
    out, res = fn(c, cs, dt, ds)
    _check(mix, res.cpu().numpy(), out.cpu().numpy())
    for it in items:
        c, cs, dt, ds = rc.huf_device_batch([it[0]], torch)
        out, res = fn(c, cs, dt, ds)
        _check([it], res.cpu().numpy(), out.cpu().numpy())


def test_shared_table_batch(hip, corpus):
    """five blocks behind ONE table (table stride 0), dispatching and strict call, max_table_log 12 and 11 (a table of log 12)"""
    items = [it for it in corpus if "shared_table" in it[0].labels]
    assert len(items) == 5 and all((it[0].dt == items[0][0].dt).all() for it in items)
    c, cs, dt, ds = rc.huf_device_batch([e for e, _ in items], torch)
    for L in (12, 11):
        for fn in _fns(hip, 4):
            out, res = fn(c, cs, dt[:1], ds, max_table_log=L, shared_table=True)
            _check(items, res.cpu().numpy(), out.cpu().numpy(), L)
    assert all(it[1][12][0] == it[0].dst_size for it in items)
