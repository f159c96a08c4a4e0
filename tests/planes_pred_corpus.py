"""The numpy model of the predicted planes (include/fsehip.h, "predicted planes") shared by test_planes_pred_model.py and
test_gpu_planes_pred.py, built on planes_corpus.py and planes_sub_corpus.py: the predicted split is the split of
z[j] = zigzag(t[j] - p[j]), p[j] = 0 where j mod RUN == 0 and t[j - 1] elsewhere; the predicted merge sums every run of unzigzag(z) back.
Elements are little-endian unsigned integers of E bytes counted from the tensor's start; the trailing n mod E bytes pass unchanged.
Plain Python, never the library.  Tensors are numpy uint8 arrays."""
import numpy as np

import planes_corpus as pc
import planes_sub_corpus as psc

RUN_LOG = 10                   # FSEHIP_PRED_RUN_LOG
RUN = 1 << RUN_LOG
_U = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}


def forward(t, E):
    """the bytes of z, element by element"""
    t = np.ascontiguousarray(t, np.uint8)
    assert t.ndim == 1
    whole = len(t) // E * E
    out = t.copy()
    x = t[:whole].view(_U[E])
    prev = np.zeros_like(x)
    prev[1:] = x[:-1]
    prev[::RUN] = 0
    with np.errstate(over="ignore"):
        out[:whole] = psc._zz(x, prev, E).view(np.uint8)
    return out


def inverse(z, E):
    """the tensor whose differences are z"""
    z = np.ascontiguousarray(z, np.uint8)
    assert z.ndim == 1
    whole = len(z) // E * E
    out = z.copy()
    x = z[:whole].view(_U[E])
    m = len(x)
    with np.errstate(over="ignore"):
        d = psc._unzz(x, np.zeros_like(x), E)
        pad = np.zeros(-(-m // RUN) * RUN, d.dtype)
        pad[:m] = d
        t = np.cumsum(pad.reshape(-1, RUN), axis=1, dtype=d.dtype).reshape(-1)[:m]       # (the sums wrap in the element's width)
    assert t.dtype == x.dtype
    out[:whole] = t.view(np.uint8)
    return out


def pred_all(tensors, E):
    """what the planes of a *_pred_dbatch call are the planes of"""
    return [forward(t, E) for t in tensors]


def split_pred_model(tensors, E, capacity=None):
    """-> (planes buffer, written, plane offsets, tensor results) of FSEHIP_planes_split_pred_dbatch"""
    return pc.split_model(pred_all(tensors, E), E, capacity)


def merge_pred_one(planes, E):
    """the tensor whose predicted planes these are"""
    return inverse(pc.merge_one(planes, E), E)


def edge_values(E):
    return psc.edge_values(E)


def edge_sequence(E, lead=0):
    """elements as bytes: `lead` filler elements, then every ordered pair over edge_values(E) as neighbours, x y x -- the difference wraps
    upwards and downwards next to each other.  `lead` moves the pairs across lane (16), run (1024) and tile boundaries"""
    vals = edge_values(E)
    seq = [(7 * k + 3) % 251 for k in range(lead)]
    for x in vals:
        for y in vals:
            seq += [x, y, x]
    return np.array(seq, dtype=np.uint64).astype(_U[E]).view(np.uint8).copy()
