"""Differentiable augmentation of the discriminator's inputs (Trainer.diffaug; pg_diffaug_params / _fwd / _bwd of diffaug.hip) restated
without the library: the parameter draw in Python integers (exact), the map and its adjoint in NumPy, and an OracleTrainer whose
discriminator reads the augmented tensors through differentiable torch indexing, so torch autograd supplies the gradient through the
map.  Pure CPU: nothing here calls the library.

A table is an int array [N, 8]: rows {flip, ty, tx, cut_top, cut_left, cut_h, cut_w, 0} (include/patchgan_hip.h).  The map, per output
pixel (h, w) of sample n:  inside the box -> 0;  hs = h - ty, ws = w - tx, outside the image -> 0;  flipped: ws = W - 1 - ws;
out[n, h, w] = x[n, hs, ws].  It is an injective partial map of pixels: the adjoint scatters every g element to at most one place and
no two to the same one."""
import itertools

import numpy as np
import torch

from oracle.patchgan_oracle import OracleTrainer

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
DOMAIN = 0x6469666661756721
FLIP, TRANSLATION, CUTOUT = 1, 2, 4
NAMES = {'flip': FLIP, 'translation': TRANSLATION, 'cutout': CUTOUT}
POLICIES = tuple(range(8))                                   # every subset of the three bits
POLICY_NAMES = {p: ','.join(n for n, b in NAMES.items() if p & b) for p in POLICIES}
NEUTRAL_ROW = (0, 0, 0, 0, 0, 0, 0, 0)


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def draw(seed, t, s, k):
    """Draw k of global sample s at step count t of stream `seed`: a 64-bit integer."""
    key = mix64(mix64(((seed ^ DOMAIN) + GOLD * (t + 1)) & M64) + GOLD * (s + 1))
    return mix64(key + GOLD * (k + 1))


def params_ref(seed, t, policy, sample0, N, H, W):
    """The table pg_diffaug_params writes, as an int32 array [N, 8]."""
    out = np.zeros((N, 8), dtype=np.int32)
    for n in range(N):
        s = sample0 + n
        if policy & FLIP:
            out[n, 0] = draw(seed, t, s, 0) >> 63
        if policy & TRANSLATION:
            out[n, 1] = (draw(seed, t, s, 1) >> 32) % (2 * (H // 8) + 1) - H // 8
            out[n, 2] = (draw(seed, t, s, 2) >> 32) % (2 * (W // 8) + 1) - W // 8
        if policy & CUTOUT:
            ch, cw = H // 2, W // 2
            out[n, 3] = (draw(seed, t, s, 3) >> 32) % (H + 1) - ch // 2
            out[n, 4] = (draw(seed, t, s, 4) >> 32) % (W + 1) - cw // 2
            out[n, 5], out[n, 6] = ch, cw
    return out


def masked(table, policy):
    """A hand-made table with the columns of the policy bits that are off set to their neutral values."""
    t = np.array(table, dtype=np.int32).copy()
    if not policy & FLIP:
        t[:, 0] = 0
    if not policy & TRANSLATION:
        t[:, 1:3] = 0
    if not policy & CUTOUT:
        t[:, 3:7] = 0
    return t


def extreme_tables(N, H, W):
    """Hand-made tables [N, 8]: the largest shifts of both signs, boxes hanging over each border, a box that covers nothing and one
    that lies wholly inside, flips on and off.  Sample n takes row n % len(rows) of each list."""
    my, mx, ch, cw = H // 8, W // 8, H // 2, W // 2
    a = [(1, my, mx, -(ch // 2), -(cw // 2), ch, cw, 0),                   # down / right, box over the top-left corner
         (0, -my, -mx, H - ch // 2, W - cw // 2, ch, cw, 0),               # up / left, box over the bottom-right corner
         (1, -my, mx, -(ch // 2), W - cw // 2, ch, cw, 0),                 # box over the top-right corner
         (0, my, -mx, H - ch // 2, -(cw // 2), ch, cw, 0),                 # box over the bottom-left corner
         (1, 0, 0, (H - ch) // 2, (W - cw) // 2, ch, cw, 0)]               # no shift, box inside
    b = [(1, my, -mx, 0, 0, 0, 0, 0),                                      # the empty box
         (0, -my, mx, 1, 1, ch, cw, 0),
         (1, 1, -1, H - 1, W - 1, ch, cw, 0),                              # one pixel of box inside
         (0, 0, 0, -ch + 1, -cw + 1, ch, cw, 0)]
    return [np.array([rows[(n + i) % len(rows)] for n in range(N)], dtype=np.int32) for i, rows in ((0, a), (1, a), (0, b))]


def _source_index(row, H, W):
    """(ok [H, W] bool, hs [H, W], ws [H, W]): for every output pixel of the map, whether it copies and from where."""
    flip, ty, tx, top, left, bh, bw = (int(v) for v in row[:7])
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    box = (h >= top) & (h < top + bh) & (w >= left) & (w < left + bw)
    hs, ws = h - ty, w - tx
    ok = ~box & (hs >= 0) & (hs < H) & (ws >= 0) & (ws < W)
    if flip:
        ws = W - 1 - ws
    return ok, np.where(ok, hs, 0), np.where(ok, ws, 0)


def apply(x, params):
    """The map on an NHWC array [N, H, W, C]: values are moved or replaced by +0, never computed on."""
    N, H, W, _ = x.shape
    out = np.zeros_like(x)
    for n in range(N):
        ok, hs, ws = _source_index(params[n], H, W)
        out[n][ok] = x[n][hs[ok], ws[ok]]
    return out


def adjoint(g, params):
    """The transpose of apply: g[n, h, w] goes to the one source pixel output (h, w) copied from; every other element is +0."""
    N, H, W, _ = g.shape
    out = np.zeros_like(g)
    for n in range(N):
        ok, hs, ws = _source_index(params[n], H, W)
        out[n][hs[ok], ws[ok]] = g[n][ok]          # (injective: no index pair occurs twice)
    return out


def apply_torch(x, params):
    """The same map on an NCHW torch tensor by differentiable indexing (autograd's gradient through it is the adjoint)."""
    N, _, H, W = x.shape
    outs = []
    for n in range(N):
        ok, hs, ws = _source_index(np.asarray(params[n]), H, W)
        picked = x[n][:, torch.as_tensor(hs), torch.as_tensor(ws)]
        outs.append(torch.where(torch.as_tensor(ok)[None], picked, torch.zeros((), dtype=x.dtype)))
    return torch.stack(outs)


class AugOracleTrainer(OracleTrainer):
    """OracleTrainer whose discriminator reads T(x | y) and T(x | G(x)): all three D calls of batch() see the map with the table in
    `self.table` ([N, 8]; None = no augmentation), real and fake sample i under the same row."""

    table = None

    def D(self, x, probes=None):
        if self.table is not None:
            x = apply_torch(x, self.table)
        return super().D(x, probes)


def subsets():
    return list(itertools.chain.from_iterable(itertools.combinations(NAMES, r) for r in range(4)))


def find_seed(N, H, W, t=0, policy=FLIP | TRANSLATION | CUTOUT, sample0=0, limit=100000):
    """The smallest seed whose table at step count t gives EVERY sample flip = 1, non-zero ty and tx, and a box that zeroes some but
    not all of the image."""
    for seed in range(limit):
        p = params_ref(seed, t, policy, sample0, N, H, W)
        if all(interesting(r, H, W) for r in p):
            return seed
    raise AssertionError('no seed found')


def interesting(row, H, W):
    flip, ty, tx, top, left, bh, bw = (int(v) for v in row[:7])
    rows = max(0, min(H, top + bh) - max(0, top))
    cols = max(0, min(W, left + bw) - max(0, left))
    return flip == 1 and ty != 0 and tx != 0 and 0 < rows * cols < H * W
