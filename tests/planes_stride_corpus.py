"""The numpy model of the strided predicted planes (include/fsehip.h, "strided predicted planes") shared by test_planes_stride_model.py and
test_gpu_planes_stride.py, built on planes_corpus.py, planes_sub_corpus.py and planes_pred_corpus.py: the strided split is the split of
z[j] = zigzag(t[j] - p[j]), p[j] = 0 where (j mod RUN) < S and t[j - S] elsewhere; the strided merge sums the S interleaved chains of every
run of unzigzag(z) back -- the chain of an element is (j mod RUN) mod S, it starts again with every run.  Elements are little-endian
unsigned integers of E bytes counted from the tensor's start; the trailing n mod E bytes pass unchanged.  And the five interleaved corpora
the feature is for, 2^18 elements each, seeds and sizes fixed.  Plain Python, never the library.  Tensors are numpy uint8 arrays."""
import numpy as np

import planes_corpus as pc
import planes_pred_corpus as ppc
import planes_sub_corpus as psc

RUN = ppc.RUN
MAX_STRIDE = 8                 # FSEHIP_PRED_MAX_STRIDE
STRIDES = tuple(range(1, MAX_STRIDE + 1))
_U = ppc._U


def forward(t, E, S):
    """the bytes of z, element by element"""
    t = np.ascontiguousarray(t, np.uint8)
    assert t.ndim == 1 and 1 <= S <= MAX_STRIDE
    whole = len(t) // E * E
    out = t.copy()
    x = t[:whole].view(_U[E])
    prev = np.zeros_like(x)
    prev[S:] = x[:-S]
    prev[np.arange(len(x)) % RUN < S] = 0
    with np.errstate(over="ignore"):
        out[:whole] = psc._zz(x, prev, E).view(np.uint8)
    return out


def inverse(z, E, S):
    """the tensor whose strided differences are z"""
    z = np.ascontiguousarray(z, np.uint8)
    assert z.ndim == 1 and 1 <= S <= MAX_STRIDE
    whole = len(z) // E * E
    out = z.copy()
    x = z[:whole].view(_U[E])
    m = len(x)
    with np.errstate(over="ignore"):
        d = psc._unzz(x, np.zeros_like(x), E)
        pad = np.zeros((-(-m // RUN), RUN), d.dtype)
        pad.reshape(-1)[:m] = d
        for a in range(S):                                     # chain a of every run: the positions a, a + S, .. of the run
            pad[:, a::S] = np.cumsum(pad[:, a::S], axis=1, dtype=d.dtype)      # (the sums wrap in the element's width)
    out[:whole] = pad.reshape(-1)[:m].view(np.uint8)
    return out


def pred_all(tensors, E, S):
    """what the planes of a *_pred_stride_dbatch call are the planes of"""
    return [forward(t, E, S) for t in tensors]


def split_model(tensors, E, S, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_pred_stride_dbatch"""
    return pc.split_model(pred_all(tensors, E, S), E, capacity)


def edge_values(E):
    """the edge values of the arithmetic deltas, and for E == 8 the two sides of the dword boundary"""
    vals = list(psc.edge_values(E))
    for v in ((1 << 32) - 1, 1 << 32) if E == 8 else ():
        if v not in vals:
            vals.append(v)
    return vals


def across(E, S, period):
    """every ordered pair (x, y) of edge values as STRIDE-neighbours across a boundary, on a smooth ramp: pair k occupies the S elements in
    front of the boundary period * (k + 1) with x and the S elements behind it with y, so that every one of the positions
    period - S .. period - 1 | period .. period + S - 1 holds an edge value whose stride-neighbour is one too.  period 16: lane boundaries
    (y is predicted by x); 1024: run boundaries (y is a chain head, x closes its chains)"""
    vals = edge_values(E)
    pairs = [(x, y) for x in vals for y in vals]
    seq = (np.arange(period * (len(pairs) + 1) + 3, dtype=np.uint64) * np.uint64(3)) & np.uint64((1 << (8 * E - 1)) - 1 if E < 8 else (1 << 40) - 1)
    for k, (x, y) in enumerate(pairs):
        b = period * (k + 1)
        seq[b - S:b], seq[b:b + S] = x, y
    return seq.astype(_U[E]).view(np.uint8).copy()


def channels(E, S, m):
    """m elements whose channel c = (j mod S) holds c + 1 everywhere"""
    return (np.arange(m, dtype=np.uint64) % np.uint64(S) + np.uint64(1)).astype(_U[E]).view(np.uint8).copy()


# ---- the five corpora: (name, E, S, bytes), 2^18 elements each -------------------------------------------------------------------------------
N = 1 << 18


def stereo():
    """int16 stereo: two different random walks, interleaved"""
    rng = np.random.default_rng(11)
    left = np.cumsum(rng.integers(-40, 41, N // 2))
    right = 3000 + np.cumsum(rng.integers(-25, 26, N // 2))
    return np.stack([left, right], axis=1).reshape(-1).astype(np.int16).view(np.uint8).copy()


def rgb():
    """uint8 RGB: smooth rows, each channel around a level of its own, and a little noise"""
    rng = np.random.default_rng(12)
    k = np.arange(-(-N // 3))
    px = np.stack([60 + 40 * np.sin(k / 90.0), 128 + 50 * np.sin(k / 150.0 + 1), 200 + 30 * np.sin(k / 60.0 + 2)], axis=1)
    px = np.rint(px + rng.integers(-1, 2, px.shape)).clip(0, 255)
    return px.reshape(-1)[:N].astype(np.uint8).copy()


def xyz():
    """float32 xyz: a random-walk trajectory, each axis around an offset of its own"""
    rng = np.random.default_rng(13)
    m = -(-N // 3)
    pos = np.array([100.0, -37.0, 5.5]) + np.cumsum(rng.standard_normal((m, 3)) * 1e-4, axis=0)
    return pos.reshape(-1)[:N].astype(np.float32).view(np.uint8).copy()


def boxes():
    """int32 boxes (x, y, w, h): x sorted, y a slow walk, w and h near sizes of their own"""
    rng = np.random.default_rng(14)
    m = N // 4
    x = np.sort(rng.integers(0, 1 << 24, m))
    y = 500 + np.cumsum(rng.integers(-3, 4, m))
    w = 64 + rng.integers(0, 8, m)
    h = 200 + rng.integers(0, 16, m)
    return np.stack([x, y, w, h], axis=1).reshape(-1).astype(np.int32).view(np.uint8).copy()


def phasor():
    """complex64 seen as pairs of float32: a slow phasor of slowly changing amplitude"""
    rng = np.random.default_rng(15)
    m = N // 2
    phase = np.cumsum(2e-4 + 1e-6 * rng.standard_normal(m))
    amp = 1.0 + 0.1 * np.sin(np.arange(m) / 5000.0)
    z = (amp * np.exp(1j * phase)).astype(np.complex64)
    return z.view(np.float32).view(np.uint8).copy()


CORPORA = (("int16 stereo", 2, 2, stereo), ("uint8 RGB", 1, 3, rgb), ("float32 xyz", 4, 3, xyz), ("int32 boxes", 4, 4, boxes),
           ("complex64 phasor", 4, 2, phasor))
