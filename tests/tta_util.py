"""The arithmetic of tiled inference with test-time augmentation and a blend window, in plain NumPy loops: the independent statement the
host restatement (infer.n_crop / build_mask) and the kernels (pg_tiles_gather_tta / pg_tiles_blend_win) are held to bit for bit.
Nothing here calls the package: tile starts, variant maps and window tables are written out again."""
import numpy as np

TTA_NAME = {1: None, 2: 'hflip', 4: 'flips', 8: 'd4'}

# the two smallest tiled shapes: clamped and duplicate tiles on both axes (size 8: rows 0 5 5, columns 0 6 11 11), odd tile size
SHAPES = [(3, 13, 19, 8, 0.75), (3, 13, 19, 7, 0.75)]


def starts(extent, size, eff):
    return [min(k * eff, extent - size) for k in range(-(-extent // eff))]


def variant(tile, k):
    """Variant k of a [..., size, size] array: transpose if k & 4, then flip rows if k & 2, then flip columns if k & 1."""
    if k & 4:
        tile = np.swapaxes(tile, -1, -2)
    if k & 2:
        tile = tile[..., ::-1, :]
    if k & 1:
        tile = tile[..., :, ::-1]
    return tile


def inverse_positions(k, size):
    """pos[ty, tx] = (y, x): where position (ty, tx) of a tile sits in its variant k, found by pushing an index grid through variant()."""
    grid = variant(np.arange(size * size).reshape(size, size), k)
    pos = np.zeros((size, size, 2), dtype=np.int64)
    for y in range(size):
        for x in range(size):
            pos[grid[y, x] // size, grid[y, x] % size] = (y, x)
    return pos


def window(name, size):
    if name is None:
        return np.ones(size)
    if name == 'pyramid':
        return np.array([float(min(u + 1, size - u)) for u in range(size)])
    if name == 'hann':
        return np.sin(np.pi * (np.arange(size) + 0.5) / size) ** 2
    return np.asarray(name, dtype=np.float64)


def crops_ref(image, size, overlap, K):
    """[K * T, C, size, size]: variant k of tile t at k * T + t, tiles row-major."""
    c, H, W = image.shape
    eff = int(overlap * size)
    ys, xs = starts(H, size, eff), starts(W, size, eff)
    out = []
    for k in range(K):
        for sy in ys:
            for sx in xs:
                out.append(variant(image[:, sy:sy + size, sx:sx + size], k))
    return np.stack(out)


def blend_ref(pred, size, image_size, overlap, K, win, threshold):
    """pred [K * T, C, size, size] float32 -> (average [C, H, W] float64, what build_mask returns).  One pixel at a time: tiles
    ascending, variants ascending inside, one rounded product per weight and per term, one rounded sum."""
    pred = np.asarray(pred)
    C = pred.shape[1]
    H, W = image_size
    eff = int(overlap * size)
    ys, xs = starts(H, size, eff), starts(W, size, eff)
    T = len(ys) * len(xs)
    assert pred.shape[0] == K * T
    win = np.asarray(win, dtype=np.float64)
    pos = [inverse_positions(k, size) for k in range(K)]
    avg = np.zeros((C, H, W))
    for h in range(H):
        for w in range(W):
            acc, wsum = np.zeros(C), np.float64(0.0)
            for j, sy in enumerate(ys):
                for i, sx in enumerate(xs):
                    if not (sy <= h < sy + size and sx <= w < sx + size):
                        continue
                    wgt = win[h - sy] * win[w - sx]
                    for k in range(K):
                        y, x = pos[k][h - sy, w - sx]
                        term = wgt * pred[k * T + j * len(xs) + i, :, y, x].astype(np.float64)
                        acc = acc + term
                        wsum = wsum + wgt
            avg[:, h, w] = acc / wsum
    out = (avg >= threshold).astype(np.float64) if threshold > 0 else avg
    return avg, (np.argmax(out, axis=0) if C > 1 else out[0])
