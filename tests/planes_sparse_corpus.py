"""The numpy model of sparse planes (include/fsehip.h, "sparse planes") shared by test_planes_sparse_model.py and test_gpu_planes_sparse.py: a
unit of n bytes as a zero mask of ceil(n / 8) bytes followed by its non-zero bytes where the writer rule says so, the unit itself otherwise,
and the reader rule that tells the two apart by the content's size alone.  Plain Python, never the library.  Units and contents are numpy
uint8 arrays; error results are negative ints (-c for error code c), as the binding shows them."""
import numpy as np

import planes_corpus as pc
from planes_corpus import CORRUPT

TILE = pc.TILE                # bytes of the flat axis per work item of the pack and expand kernels (csrc/internal.h: PLANES_TILE)
# Recorded: frame bytes, low plane + high plane, of the bf16 update pair of planes_delta_corpus.py at block-size id 5 -- {(delta, codec):
# (the planes themselves, their sparse contents at permille 500)}, from the CPU oracle
TABLE = {("xor", 0): (69334, 68118), ("xor", 1): (103787, 71779), ("sub", 0): (59915, 58867), ("sub", 1): (95708, 63411)}


def mask_bytes(n):
    return (int(n) + 7) // 8


def is_sparse(n, nnz, permille):
    """the writer rule, in Python's unbounded integers"""
    return nnz * 1000 <= n * permille and mask_bytes(n) + nnz < n


def pack_unit(unit, permille):
    """-> the content of one unit"""
    unit = np.ascontiguousarray(unit, np.uint8)
    n, nz = len(unit), unit != 0
    if not is_sparse(n, int(nz.sum()), permille):
        return unit.copy()
    mask = np.packbits(nz, bitorder="little")                 # bit i & 7 of byte i >> 3, padding bits zero
    assert len(mask) == mask_bytes(n)
    return np.concatenate([mask, unit[nz]])


def expand_unit(content, n):
    """-> (result, unit or None): the reader rule for a unit of n bytes.  `content` is the content the frame reader regenerated, or its
    (negative) error"""
    if isinstance(content, (int, np.integer)):
        assert content < 0
        return int(content), None
    content = np.ascontiguousarray(content, np.uint8)
    c, m = len(content), mask_bytes(n)
    if c == n:
        return n, content.copy()
    if c > n or c < m:
        return CORRUPT, None
    bits = np.unpackbits(content[:m], bitorder="little")
    values = content[m:]
    if int(bits.sum()) != c - m or bits[n:].any() or not values.all():
        return CORRUPT, None
    unit = np.zeros(n, np.uint8)
    unit[bits[:n].astype(bool)] = values
    return n, unit


def pack_model(units, permille):
    """-> (contents, content offsets) of FSEHIP_sparse_pack_dbatch over units laid back to back"""
    contents = [pack_unit(u, permille) for u in units]
    return contents, [int(x) for x in pc.offsets(contents)]


def cut(buf, offsets):
    """the units of a flat buffer by an offsets list (non-increasing pairs are empty units)"""
    return [buf[int(a):max(int(a), int(b))] for a, b in zip(offsets[:-1], offsets[1:])]


def flip_permille(n_a, nnz_a, n_b, nnz_b):
    """a permille at which unit a is sparse and unit b is not (None if there is none): the smallest one that admits a"""
    for p in range(1001):
        if is_sparse(n_a, nnz_a, p):
            return None if is_sparse(n_b, nnz_b, p) else p
    return None


def with_density(n, nnz, seed, lo=1, hi=256):
    """a unit of n bytes with exactly nnz non-zero bytes at random places"""
    rng = np.random.default_rng(seed)
    u = np.zeros(n, np.uint8)
    u[rng.permutation(n)[:nnz]] = rng.integers(lo, hi, nnz, dtype=np.uint8)
    return u


def damaged_contents(unit):
    """[(name, content, n)] for every refusal of the reader rule, made from the sparse content of `unit` (which must be sparse at permille
    1000, have a partial last mask byte, a zero byte somewhere and at least one value)"""
    n, m = len(unit), mask_bytes(len(unit))
    good = pack_unit(unit, 1000)
    assert m < len(good) < n and n % 8 and not unit.all()
    out = [("longer than the unit", np.ones(n + 1, np.uint8), n), ("shorter than the mask", good[:m - 1].copy(), n)]
    more = np.concatenate([good, [7]]).astype(np.uint8)                       # one value more than the mask has bits
    out.append(("popcount one short", more, n))
    out.append(("popcount one over", good[:-1].copy(), n))
    pad = good.copy()
    pad[m - 1] |= 0x80                                                        # a padding bit, and a value for it: the popcount agrees
    out.append(("a padding bit", np.concatenate([pad, [9]]).astype(np.uint8), n))
    zero = good.copy()
    zero[m] = 0
    out.append(("a zero among the values", zero, n))
    for name, c, k in out:
        assert expand_unit(c, k) == (CORRUPT, None), name
    return out
