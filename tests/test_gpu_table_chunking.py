"""The table-building batch calls walk a batch in passes when the caller's workspace holds fewer blocks than the batch, like the one-shot
calls (test_gpu_chunking.py).  Each call is run with the workspace its size function asks for and with a workspace for exactly one
block -- one pass per block -- and must leave bit-identical tables, headers and results.  A workspace one byte below what one block
needs is refused before anything is launched.  The thresholds are spelled out here, from the per-block scratch of each call (record,
counters, lists) plus the 2048 bytes of slack every workspace carries, rather than taken from the library."""
import ctypes as C

import pytest
import torch

from finitestateentropy_amd.api import SZ, _ptr, _stream

pytestmark = pytest.mark.gpu

SIZE = 1024
SENTINEL = 0x5A
# bytes one block needs: per-block scratch + slack
FSE_META, HUF_META, SLACK = 20, 16, 2048
NEED = {
    "FSE_buildCTable": 1024 + 4 + 8 + FSE_META + SLACK,                               # 256 counters, largest symbol, histogram result, record
    "FSE_buildDTable": FSE_META + 512 + 3 * (1 << 12) + 48 * 4 + SLACK,               # record, 256 norms, 2 + 1 bytes per cell at maxLog 12, 48 class lists
    "HUF_buildCTable": 1024 + 4 + 8 + HUF_META + SLACK,
    "HUF_readDTableX1": HUF_META + 8 * 4 + SLACK,                                     # record, 8 class lists
    "HUF_readDTableX2": HUF_META + 8 * 4 + SLACK,
}


@pytest.fixture(scope="module")
def corpus(hip):
    """5 blocks of 1 KiB, three skews mixed, then an all-equal block and a 1-byte block; their FSE headers and Huff0 blocks for the readers"""
    src = torch.zeros((7, SIZE), dtype=torch.uint8, device="cuda")
    hip.probagen_mixed((2, 14, 80), 5, SIZE, out=src[:5])
    src[5] = 0x41
    src[6, 0] = 0x42
    sizes = torch.tensor([SIZE] * 6 + [1], dtype=torch.int64, device="cuda")
    _, hdr, hres = hip.fse_build_ctable_batch(src[:5].contiguous(), table_log=12)
    comp, cres = hip.huf_compress_batch(src[:5].contiguous())
    torch.cuda.synchronize()
    assert bool((hres > 1).all()), hres                     # every mixed block has an NCount header
    assert int((cres > 1).sum()) >= 3, cres                 # and most of them a Huff0 block with a weight header
    return {"src": src, "sizes": sizes, "hdr": hdr.contiguous(), "hres": hres.clone(), "comp": comp.contiguous(), "cres": cres.clone()}


def _ws_size(hip, name, n):
    fn = getattr(hip.lib, "FSEHIP_%s_batch_workspaceSize" % name)
    fn.restype = C.c_size_t
    return int(fn(SZ(n), C.c_uint(12)) if name == "FSE_buildDTable" else fn(SZ(n)))


def _call(hip, name, c, ws_bytes, fill):
    """one call of FSEHIP_<name>_batch on the corpus with a workspace of ws_bytes; outputs start as `fill`.  -> (return code, outputs)"""
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    fn = getattr(hip.lib, "FSEHIP_%s_batch" % name)
    fn.restype = C.c_int
    if name in ("FSE_buildCTable", "HUF_buildCTable"):
        n, ctw = 7, (1 + (1 << 11) + 512 if name[0] == "F" else 256)
        ct = torch.full((n, ctw), fill, dtype=torch.int32, device="cuda")
        hdr = torch.full((n, 512), fill, dtype=torch.uint8, device="cuda")
        res = torch.full((n,), fill, dtype=torch.int64, device="cuda")
        rc = fn(_ptr(ct), SZ(ctw), _ptr(hdr), SZ(512), SZ(512), _ptr(res), _ptr(c["src"]), SZ(SIZE), _ptr(c["sizes"]), SZ(0),
                C.c_uint(255), C.c_uint(12 if name[0] == "F" else 11), SZ(n), _ptr(ws), SZ(ws_bytes), _stream())
        out = (ct, hdr, res)
    else:
        n = 5
        dt = torch.full((n, 1 + (1 << 12)), fill, dtype=torch.int32, device="cuda")
        res = torch.full((n,), fill, dtype=torch.int64, device="cuda")
        if name == "FSE_buildDTable":
            rc = fn(_ptr(dt), SZ(dt.stride(0)), _ptr(res), _ptr(c["hdr"]), SZ(c["hdr"].stride(0)), _ptr(c["hres"]), SZ(0),
                    C.c_uint(12), SZ(n), _ptr(ws), SZ(ws_bytes), _stream())
        else:
            rc = fn(_ptr(dt), SZ(dt.stride(0)), C.c_uint(12), _ptr(res), _ptr(c["comp"]), SZ(c["comp"].stride(0)), _ptr(c["cres"]), SZ(0),
                    SZ(n), _ptr(ws), SZ(ws_bytes), _stream())
        out = (dt, res)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", sorted(NEED))
def test_one_block_workspace_same_tables(hip, corpus, name):
    n = 7 if name.endswith("buildCTable") else 5
    assert _ws_size(hip, name, 1) == NEED[name]
    rc0, full = _call(hip, name, corpus, _ws_size(hip, name, n), 0)
    rc1, one = _call(hip, name, corpus, NEED[name], 0)             # room for one block: a pass per block
    assert rc0 == 0 and rc1 == 0
    for a, b in zip(full, one):
        assert torch.equal(a, b)
    res = full[-1]
    if n == 7:
        good = (res[:5] > 1) & (res[:5] < 512)                                                # header sizes
        assert int(good.sum()) >= (5 if name[0] == "F" else 3) and int(res[5]) <= 1 and int(res[6]) <= 1, res   # one symbol / one byte: no header
        assert bool((full[0][:5][good] != 0).any(dim=1).all())                                # a table behind every header
    else:
        ok = (corpus["cres"] > 1) if name.startswith("HUF") else torch.ones(5, dtype=torch.bool, device="cuda")
        assert bool(((res > 1) & (res < 512))[ok].all()), res                                 # header sizes
        assert bool((full[0][ok] != 0).any(dim=1).all())


@pytest.mark.parametrize("name", sorted(NEED))
def test_workspace_below_one_block_is_refused(hip, corpus, name):
    rc, out = _call(hip, name, corpus, NEED[name] - 1, SENTINEL)
    assert rc != 0
    for t in out:                                                  # nothing was launched: every output is as it was
        assert bool((t == SENTINEL).all())
