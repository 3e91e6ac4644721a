"""The semantics of pg_seg_hist and metrics.curve in NumPy, written independently of both (np.floor on the fp32 product, np.argmax,
np.add.at; thresholds applied to the predictions directly, no cumulative sums), and the edge-value recipe of the histogram tests."""
import numpy as np


def hist_ref(p_nchw, y_nchw, bins):
    """(hist np.int64 [C, 2, bins], ignored int) of prediction p against target y, both [N, C, H, W] float32.
    bin: bins-1 where p >= 1, 0 where p <= 0, floor(p * bins) in fp32 elsewhere.
    label: C == 1: y >= 0.5, nothing ignored.  C > 1: channel == np.argmax(y) (one-vs-rest); a pixel whose largest y is <= 0 is
    ignored.  hist[c, t, b] counts the kept pixels of channel c with label t in bin b."""
    p = np.asarray(p_nchw, dtype=np.float32)
    y = np.asarray(y_nchw, dtype=np.float32)
    assert p.shape == y.shape and p.ndim == 4
    N, C, H, W = p.shape
    b = np.floor(p * np.float32(bins))
    assert b.dtype == np.float32
    b = np.where(p >= np.float32(1), bins - 1, np.where(p <= np.float32(0), 0, b)).astype(np.int64)
    if C == 1:
        t = (y >= np.float32(0.5)).astype(np.int64)
        keep = np.ones((N, H, W), dtype=bool)
    else:
        lab = np.argmax(y, axis=1)
        t = (np.arange(C)[None, :, None, None] == lab[:, None]).astype(np.int64)
        keep = y.max(axis=1) > 0
    hist = np.zeros((C, 2, bins), dtype=np.int64)
    for c in range(C):
        np.add.at(hist[c], (t[:, c][keep], b[:, c][keep]), 1)
    return hist, int((~keep).sum())


def curve_ref(p_nchw, y_nchw, bins):
    """{'tp', 'fp', 'fn', 'tn'}: int64 [C, bins], the counts at every threshold k / bins found by thresholding p >= float32(k / bins)
    directly for k >= 1 (labels and the ignore rule as in hist_ref); threshold 0 takes every kept pixel."""
    p = np.asarray(p_nchw, dtype=np.float32)
    y = np.asarray(y_nchw, dtype=np.float32)
    N, C, H, W = p.shape
    if C == 1:
        t = y >= np.float32(0.5)
        keep = np.ones((N, H, W), dtype=bool)
    else:
        t = np.arange(C)[None, :, None, None] == np.argmax(y, axis=1)[:, None]
        keep = y.max(axis=1) > 0
    out = {k: np.zeros((C, bins), dtype=np.int64) for k in ('tp', 'fp', 'fn', 'tn')}
    for c in range(C):
        pc, tc = p[:, c][keep], t[:, c][keep]
        for k in range(bins):
            # (k = 0 predicts every pixel: the clamp puts a prediction below 0 into the first bin, which p >= 0 would leave out)
            q = pc >= np.float32(k / bins) if k else np.ones(pc.shape, dtype=bool)
            out['tp'][c, k] = np.count_nonzero(q & tc)
            out['fp'][c, k] = np.count_nonzero(q & ~tc)
            out['fn'][c, k] = np.count_nonzero(~q & tc)
            out['tn'][c, k] = np.count_nonzero(~q & ~tc)
    return out


def edge_values(bins):
    """float32 predictions around every bin border: each k / bins with its np.nextafter neighbours to both sides, the smallest
    denormal, -0.0, a value above 1, a value below 0 and the largest float below 1."""
    f = np.float32
    ks = (np.arange(bins + 1) / bins).astype(f)
    v = [ks, np.nextafter(ks, f(-2)), np.nextafter(ks, f(2)),
         np.array([1e-45, -0.0, 1.5, -0.25, np.nextafter(f(1), f(0))], dtype=f)]
    return np.concatenate(v).astype(f)


def edge_case(C, bins, seed, repeat=2):
    """(p, y) float32 [1, C, H, W] whose predictions are the edge values (every value `repeat` times per channel, shuffled per channel)
    against random targets: a 0 / 1 mask for C == 1, one-hot with about 10 % all-zero pixels otherwise."""
    rng = np.random.default_rng(seed)
    vals = np.tile(edge_values(bins), repeat)
    n = vals.size
    W = 7
    H = -(-n // W)
    p = np.zeros((1, C, H * W), dtype=np.float32)
    for c in range(C):
        fill = np.concatenate([vals, rng.choice(vals, H * W - n)])
        p[0, c] = rng.permutation(fill)
    if C == 1:
        y = (rng.random((1, 1, H * W)) > 0.6).astype(np.float32)
    else:
        lab = rng.integers(0, C, size=(1, H * W))
        y = np.zeros((1, C, H * W), dtype=np.float32)
        np.put_along_axis(y, lab[:, None], 1.0, axis=1)
        y[(rng.random((1, 1, H * W)) < 0.1).repeat(C, axis=1)] = 0.0
    return p.reshape(1, C, H, W), y.reshape(1, C, H, W)
