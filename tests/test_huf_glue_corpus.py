"""CPU pin of tests/huf_glue_corpus.py against the compiled reference: the Python restatement of the height limit gives HUF_buildCTable's lengths for
every histogram at every limit the GPU test launches (so its branch log may assign the classes), HUF_writeCTable lands where the writer model says for
every length table, every class has at least three cases, and nothing compared is undefined in the reference."""
import numpy as np

import huf_glue_corpus as C
from oracle.oracle import is_error
from test_gpu_glue_vectors import takes_m2

MIN_PER_CLASS = 3
SHAPES = {"one_symbol": lambda used, msv: used == 1, "two_symbols": lambda used, msv: used == 2, "in_use_63": lambda used, msv: used == 63,
          "in_use_64": lambda used, msv: used == 64, "in_use_65": lambda used, msv: used == 65, "msv_62": lambda used, msv: msv == 62,
          "msv_63": lambda used, msv: msv == 63, "msv_64": lambda used, msv: msv == 64, "flat_256": lambda used, msv: used == 256}


def test_height_limit_model_gives_the_reference_lengths(ref):
    """every histogram at every launch limit: table log and lengths of the model = HUF_buildCTable's; what the model declines is exactly what the
    existing tests document as undefined in the reference (more symbols than 2^limit here; the corpus has no empty histogram and no limit above 12)"""
    compared = 0
    for case in C.builder_corpus():
        count, msv = case["count"], case["msv"]
        used = int(np.count_nonzero(count[:msv + 1]))
        assert used >= 1 and msv <= 255 and int(count.max()) < 1 << 23 and not count[msv + 1:].any(), case["id"]
        for limit in C.LIMITS:
            m = C.model_build(count, msv, limit)
            if m is None:
                assert used > 1 << (limit or 11), (case["id"], limit)
                continue
            assert (limit or 11) <= 12
            tl, nb, _ = m
            r, celt = ref.huf_build_ctable(count, msv, limit)
            assert r == tl, (case["id"], limit, r, tl)
            got = ((celt >> 16) & 0xFF).astype(np.uint8)
            assert (got[:msv + 1] == nb[:msv + 1]).all(), (case["id"], limit, np.nonzero(got[:msv + 1] != nb[:msv + 1])[0][:8])
            compared += 1
    assert compared > 200, compared


def test_builder_classes_hold_and_have_three_cases_each():
    cases = C.builder_corpus()
    per_label, per_branch = {}, {b: set() for b in C.BRANCH_CLASSES}
    for case in cases:
        per_label[case["cls"]] = per_label.get(case["cls"], 0) + 1
        used = int(np.count_nonzero(case["count"][:case["msv"] + 1]))
        if case["cls"] in SHAPES:
            assert SHAPES[case["cls"]](used, case["msv"]), case["id"]
        if case["cls"] == "big_counts":
            assert int(case["count"].max()) == (1 << 23) - 1, case["id"]
        if case["cls"] == "tie_runs":                                            # long runs of equal counts
            v = np.sort(case["count"][case["count"] > 0])
            assert used - len(np.unique(v)) >= used // 2, case["id"]
        if case["cls"] == "fibonacci":
            v = np.sort(case["count"][case["count"] > 0]).astype(np.int64)
            assert (v[2:] >= v[1:-1] + v[:-2]).all(), case["id"]
        if case["at_limit"] is not None:
            assert C.builder_class(case, case["at_limit"]) == case["cls"], case["id"]
        for limit in C.LIMITS:
            cls = C.builder_class(case, limit)
            if cls in per_branch:
                per_branch[cls].add(case["id"])
    wanted = set(SHAPES) | {"tie_runs", "big_counts", "fibonacci"} | set(C.BRANCH_CLASSES)
    assert wanted <= set(per_label), wanted - set(per_label)
    for cls in wanted:
        assert per_label[cls] >= MIN_PER_CLASS, (cls, per_label[cls])
    for cls, ids in per_branch.items():
        assert len(ids) >= MIN_PER_CLASS, (cls, len(ids))
    # a cut tree that "fits" is a class of its own too: every limit must see trees that fit
    for limit in C.LIMITS:
        assert sum(C.builder_class(c, limit) == c["cls"] and c["cls"] not in C.BRANCH_CLASSES for c in cases) >= MIN_PER_CLASS, limit


# how the reference's answer shows each class: FSE-coded weights (first byte < 128), raw 4-bit weights (>= 128), the GENERIC error; a table whose
# weights took FSE_normalizeM2 may end as any of them
KIND_OF_CLASS = {"fse": ("fse",), "just_below_half": ("fse",), "one_weight": ("raw",), "no_weight_twice": ("raw",), "at_half": ("raw",), "raw": ("raw",),
                 "generic": ("generic",), "msv_0": ("raw",), "msv_1": ("raw",), "m2": ("fse", "raw", "generic")}


def _expected_header(ref, case, log):
    """(result, first byte or None) of HUF_writeCTable by the writer model"""
    msv = case["msv"]
    size, _ = C.compress_weights(ref, takes_m2, C.weights_of(case["nb"], msv, log))
    assert not is_error(size)
    if 1 < size < msv // 2:
        return size + 1, size
    if msv > 128:
        return (1 << 64) - 1, None
    return (msv + 1) // 2 + 1, (128 + msv - 1) & 0xFF


def test_writer_classes_hold_in_the_reference_and_have_three_cases_each(ref):
    """HUF_writeCTable on every length table at every launch huffLog its lengths fit: the result and the first header byte are what the model's class
    says (FSE-coded: the coded size; raw: 128 + maxSV - 1; GENERIC above 128 symbols), and at its own huffLog every table is in its labelled class"""
    per_label, compared = {}, 0
    for case in C.writer_corpus():
        nb, msv = case["nb"], case["msv"]
        assert int(nb[:msv + 1].max()) <= case["top"] and not nb[msv + 1:].any(), case["id"]
        assert C.writer_class(ref, takes_m2, case, case["at_log"]) == case["cls"], case["id"]
        per_label[case["cls"]] = per_label.get(case["cls"], 0) + 1
        for log in C.HUFF_LOGS:
            if case["top"] > log:                                                # a length above huffLog: beyond the reference's bitsToWeight[]
                continue
            r, hdr = ref.huf_write_ctable(256, C.celt_rows(nb), msv, log)
            er, first = _expected_header(ref, case, log)
            assert r == er, (case["id"], log, r, er)
            if first is not None:
                assert hdr[0] == first, (case["id"], log, hdr[0], first)
            cls = C.writer_class(ref, takes_m2, case, log)
            kind = "generic" if is_error(r) else "fse" if hdr[0] < 128 and msv >= 2 else "raw"      # (maxSV 0 writes 128 - 1: raw all the same)
            if is_error(r):
                assert r == (1 << 64) - 1
            assert kind in KIND_OF_CLASS[cls], (case["id"], log, cls, kind)
            compared += 1
    assert set(per_label) == set(C.WRITER_CLASSES), set(C.WRITER_CLASSES) ^ set(per_label)
    for cls, k in per_label.items():
        assert k >= MIN_PER_CLASS, (cls, k)
    assert compared > 80, compared


def test_refusal_lists_hold_only_what_the_reference_leaves_undefined():
    """the refusal lists never meet the reference: each entry is one of the documented cases, and the model declines the histograms"""
    for r in C.refused_hists():
        count, msv = r["count"], r["msv"]
        used = int(np.count_nonzero(count[:min(msv, 255) + 1]))
        for limit in r["limits"]:
            assert C.model_build(count, msv, limit) is None, (r["cls"], limit)
            assert used == 0 or used > 1 << (limit or 11) or msv > 255 or int(count.max()) >= 1 << 23, (r["cls"], limit)
    for r in C.refused_tables():
        for log in r["logs"]:
            assert log > 12 or r["msv"] > 255 or int(r["nb"][:r["msv"]].max()) > log, (r["cls"], log)
