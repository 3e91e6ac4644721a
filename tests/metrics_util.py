"""The semantics of pg_seg_confusion in NumPy, written independently of the kernel (np.argmax, boolean masks, np.add.at), and the
data recipe of the metric tests."""
import numpy as np


def confusion_ref(p_nchw, y_nchw, threshold):
    """(confusion np.int64 [K, K], ignored int) of prediction p against target y, both [N, C, H, W] float32.
    C == 1: predicted class = (p >= threshold), true class = (y >= 0.5), K = 2, nothing ignored.
    C  > 1: first maximum against first maximum (np.argmax), K = C; a pixel whose largest y is <= 0 is ignored.
    confusion[t, q] counts the pixels of true class t predicted as q."""
    p = np.asarray(p_nchw, dtype=np.float32)
    y = np.asarray(y_nchw, dtype=np.float32)
    assert p.shape == y.shape and p.ndim == 4
    C = p.shape[1]
    if C == 1:
        q = (p[:, 0] >= np.float32(threshold)).astype(np.int64).ravel()
        t = (y[:, 0] >= np.float32(0.5)).astype(np.int64).ravel()
        keep = np.ones(q.shape, dtype=bool)
        K = 2
    else:
        q = np.argmax(p, axis=1).ravel()
        t = np.argmax(y, axis=1).ravel()
        keep = (y.max(axis=1) > 0).ravel()
        K = C
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (t[keep], q[keep]), 1)
    return conf, int((~keep).sum())


def make_case(N, C, H, W, seed, soft=False):
    """(p, y) float32 [N, C, H, W].  Predictions are multiples of 1/8 in [0, 1]: ties between channels and values equal to a threshold
    of 0.5 or 0.25 are common.  Targets are one-hot with about 10 % of the pixels all zero (C == 1: a 0 / 1 mask), or -- soft -- random
    multiples of 1/8 (ties and all-zero pixels included)."""
    rng = np.random.default_rng(seed)
    p = (rng.integers(0, 9, size=(N, C, H, W)) / 8.0).astype(np.float32)
    if soft:
        y = (rng.integers(0, 9, size=(N, C, H, W)) / 8.0).astype(np.float32)
        y[rng.random((N, 1, H, W)).repeat(C, axis=1) < 0.1] = 0.0
    elif C == 1:
        y = (rng.random((N, 1, H, W)) > 0.7).astype(np.float32)
    else:
        lab = rng.integers(0, C, size=(N, H, W))
        y = np.zeros((N, C, H, W), dtype=np.float32)
        np.put_along_axis(y, lab[:, None], 1.0, axis=1)
        y[(rng.random((N, 1, H, W)) < 0.1).repeat(C, axis=1)] = 0.0
    return p, y
