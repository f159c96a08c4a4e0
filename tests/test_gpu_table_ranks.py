"""FSE_buildCTable / FSE_buildDTable on constructed counters, table word for table word against the COMPILED REFERENCE: the shapes that
stress the wave-cooperative spread / rank core (csrc/fse_wave_build.h) -- one cell per lane and fewer cells than lanes (tableLog 2-5),
32 and 64 cells per lane (tableLog 11 / 12), alphabets of 1, 2, 53, 64 and 65 symbols (one rank window and the first two-window one),
256 symbols, sparse alphabets, low-probability (-1) symbols, tables made only of them, and both decoder layouts (bit-reversed cells;
the plain layout of tableLog 12 tables in which one symbol holds more than half of the cells)."""
import numpy as np
import pytest
import torch

from oracle.oracle import Ref, fse_ctable_u32, fse_dtable_u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    if not Ref.available():
        pytest.skip("oracle/_ref/libfse_ref.so not built (needs the reference tree: make -C oracle ref)")
    return Ref()


def make_norm(rng, tl, nsym, nlow, sparse, big):
    """counters over `nsym` symbols (ascending positions, contiguous from 0 or spread over 0..255), `nlow` of them -1, the rest
    sharing the remaining cells (one of them more than half of the table when `big`); sum = 1 << tl with -1 counting as one"""
    ts = 1 << tl
    syms = np.sort(rng.choice(256, nsym, replace=False)) if sparse else np.arange(nsym)
    norm = np.zeros(256, dtype=np.int16)
    low = rng.choice(nsym, nlow, replace=False)
    pos = np.setdiff1d(np.arange(nsym), low)
    norm[syms[low]] = -1
    cells = ts - nlow
    if pos.size:
        share = np.ones(pos.size, dtype=np.int64)
        rest = cells - pos.size
        if big:
            top = min(ts // 2, rest)
            share[rng.integers(0, pos.size)] += top
            rest -= top
        if rest > 0:
            share += rng.multinomial(rest, rng.dirichlet(np.full(pos.size, 0.3)))
        norm[syms[pos]] = share
    assert int(np.where(norm == -1, 1, norm).sum()) == ts
    return norm, int(syms.max())


def cases(tl):
    rng = np.random.default_rng(7000 + tl)
    ts = 1 << tl
    out = []
    for nsym in (1, 2, 53, 64, 65, 256):
        if nsym > ts:
            continue
        for sparse in (False, True):
            for nlow in sorted({0, min(3, nsym - 1), min(nsym // 3, ts // 4)}):
                out.append(make_norm(rng, tl, nsym, nlow, sparse, big=False))
            if tl == 12 and nsym >= 2:                            # plain decoder layout
                out.append(make_norm(rng, tl, nsym, min(2, nsym - 1), sparse, big=True))
    if ts <= 256:                                                 # every cell a low-probability one
        out.append(make_norm(rng, tl, ts, ts, False, big=False))
    return out


@pytest.mark.parametrize("tl", [2, 4, 5, 6, 11, 12])
def test_tables_match_the_reference_cell_for_cell(hip, ref, tl):
    sets = cases(tl)
    norms = torch.from_numpy(np.stack([s[0] for s in sets])).cuda()
    msvs = torch.tensor([s[1] for s in sets], dtype=torch.int32, device="cuda")
    ct, cres = hip.fse_build_ctable_from_norm_batch(norms, msvs, tl)
    dt, dres = hip.fse_build_dtable_from_norm_batch(norms, msvs, tl)
    ct_h, dt_h = ct.cpu().numpy().view(np.uint32), dt.cpu().numpy().view(np.uint32)
    assert (cres == 0).all() and (dres == 0).all(), (cres.tolist(), dres.tolist())
    wd = fse_dtable_u32(tl)
    for i, (norm, msv) in enumerate(sets):
        rc, ect = ref.fse_build_ctable(norm, msv, tl)
        rd, edt = ref.fse_build_dtable(norm, msv, tl)
        assert rc == 0 and rd == 0, (tl, i)
        wc = fse_ctable_u32(tl, msv)
        assert (ct_h[i][:wc] == ect[:wc]).all(), (tl, i, msv, "ctable", np.nonzero(ct_h[i][:wc] != ect[:wc])[0][:8])
        assert (dt_h[i][:wd] == edt[:wd]).all(), (tl, i, msv, "dtable", np.nonzero(dt_h[i][:wd] != edt[:wd])[0][:8])


def test_plain_and_reversed_layouts_in_one_batch(hip, ref):
    """tableLog 12 counters with and without a symbol above half of the table: the two tableLog-12 decoder classes side by side"""
    rng = np.random.default_rng(7100)
    sets = [make_norm(rng, 12, n, min(2, n - 1), sparse, big) for n in (2, 53, 65, 256) for sparse in (False, True) for big in (False, True)]
    norms = torch.from_numpy(np.stack([s[0] for s in sets])).cuda()
    msvs = torch.tensor([s[1] for s in sets], dtype=torch.int32, device="cuda")
    dt, dres = hip.fse_build_dtable_from_norm_batch(norms, msvs, 12)
    dt_h = dt.cpu().numpy().view(np.uint32)
    assert (dres == 0).all()
    for i, (norm, msv) in enumerate(sets):
        rd, edt = ref.fse_build_dtable(norm, msv, 12)
        assert rd == 0 and (dt_h[i][:fse_dtable_u32(12)] == edt[:fse_dtable_u32(12)]).all(), (i, msv)
