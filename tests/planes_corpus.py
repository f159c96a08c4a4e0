"""The numpy model of the byte-plane layout (include/fsehip.h, "byte planes of tensors") shared by test_planes_model.py and test_gpu_planes.py:
plane p of a tensor is raw[p::E]; where the planes lie, what the split and the merge report, and which workgroup takes which piece -- as plain
Python, never the library.  Tensors are numpy uint8 arrays; error results are negative ints (-c for error code c), as the binding shows them."""
import numpy as np

GENERIC, TOO_SMALL, CORRUPT = -1, -2, -4
TILE = 32768                  # bytes of the flat axis per workgroup of the data kernels (csrc/internal.h: PLANES_TILE)
ELEMS = (1, 2, 4, 8)


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)


def cat(items):
    return np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(x, np.uint8) for x in items])


def plane_size(n, p, E):
    return -(-(n - p) // E) if n > p else 0


def planes_of(raw, E):
    """the E planes of one tensor"""
    return [np.asarray(raw, np.uint8)[p::E] for p in range(E)]


def split_model(tensors, E, capacity=None):
    """-> (planes buffer or None where a byte is not written, plane offsets, tensor results) of FSEHIP_planes_split_dbatch: `written` marks
    the bytes of the planes buffer the call owns"""
    S = [int(x) for x in offsets(tensors)]
    cap = S[-1] if capacity is None else int(capacity)
    out = np.zeros(S[-1], np.uint8)
    written = np.zeros(S[-1], bool)
    P, res, refused_at = [], [], None
    for i, raw in enumerate(tensors):
        if refused_at is None and S[i + 1] > cap:
            refused_at = S[i]
        if refused_at is not None:
            P += [refused_at] * E
            res.append(GENERIC)
            continue
        at = S[i]
        for p, pl in enumerate(planes_of(raw, E)):
            assert len(pl) == plane_size(len(raw), p, E)
            P.append(at)
            out[at:at + len(pl)] = pl
            written[at:at + len(pl)] = True
            at += len(pl)
        assert at == S[i + 1]
        res.append(len(raw))
    P.append(S[-1] if refused_at is None else refused_at)
    return out, written, P, res


def merge_verdict(sizes, slot_end, slot_start, E, capacity):
    """the result of one tensor of FSEHIP_planes_merge_dbatch from its E plane sizes (negative: error codes) and its slot"""
    if slot_end > capacity:
        return GENERIC
    for s in sizes:
        if s < 0:
            return s
    n = sum(sizes)
    if list(sizes) != [plane_size(n, p, E) for p in range(E)]:
        return CORRUPT
    if n > slot_end - slot_start:
        return TOO_SMALL
    return n


def merge_one(planes, E):
    """the tensor whose planes these are"""
    n = sum(len(p) for p in planes)
    raw = np.zeros(n, np.uint8)
    for p in range(E):
        raw[p::E] = planes[p]
    return raw


def work_map(S, n_groups, T=TILE):
    """the data kernels' work mapping: workgroup w takes tile t = w - i of tensor i, the largest i with S[i] // T + i <= w; it works only if the
    tensor is not empty and meets the tile.  -> list of (w, i, t) of the workgroups that work"""
    nT = len(S) - 1
    out = []
    for w in range(n_groups):
        if nT == 0 or S[0] // T > w:
            continue
        lo, hi = 0, nT - 1
        while lo < hi:
            mid = lo + ((hi - lo + 1) >> 1)
            if S[mid] // T + mid <= w:
                lo = mid
            else:
                hi = mid - 1
        i, t = lo, w - lo
        if S[i] < S[i + 1] and t * T < S[i + 1] and (t + 1) * T > S[i]:
            out.append((w, i, t))
    return out


def split_sizes(E, T=TILE):
    """the size list of the issue, in bytes, odd sizes early so that later tensors start at odd addresses"""
    return [1, E + 1, 15, 0, E - 1, E, 16 * E - 1, 16 * E, 16 * E + 1, 1024 * E - 1, 1024 * E + 1, T - 1, T, T + 1, 3 * T + 5]


def random_tensors(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(n), dtype=np.uint8) for n in sizes]


def bf16_gaussian(n, seed=1, sigma=0.02):
    """n elements of N(0, sigma) as float32 cut to their top 16 bits (bf16 by truncation), as bytes"""
    x = np.random.default_rng(seed).normal(0.0, sigma, n).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
