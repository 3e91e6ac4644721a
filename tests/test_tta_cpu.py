"""Test-time augmentation and windowed blend without a GPU: the C ABI's symbols and its argument validation (before any launch), the
window tables, and the host restatement (infer.n_crop / build_mask on CPU tensors) against the plain-NumPy loops of tests/tta_util.py,
bit for bit, at the smallest shapes with clamped and duplicate tiles."""
import os
import re

import numpy as np
import pytest
import torch

from tests import tta_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---------------------------------------------------------------------------------------------- 1. C ABI
def test_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in ('pg_tiles_gather_tta', 'pg_tiles_blend_win', 'pg_tiles_tta_max'):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.pg_tiles_tta_max() == 8


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host

    def gather(image=a, C=3, H=13, W=19, size=8, eff=6, K=8, tiles=a, ld=3):
        return lib.pg_tiles_gather_tta(image, C, H, W, size, eff, K, tiles, ld, None)

    def blend(tiles=a, ld=3, C=3, size=8, eff=6, H=13, W=19, K=8, window=a, mask=a, argmax=a):
        return lib.pg_tiles_blend_win(tiles, ld, C, size, eff, H, W, K, window, 0.5, mask, argmax, None)

    assert gather(image=None) == EINVAL and gather(tiles=None) == EINVAL
    assert blend(tiles=None) == EINVAL and blend(window=None) == EINVAL and blend(mask=None, argmax=None) == EINVAL
    for call in (gather, blend):
        for K in (0, 3, 5, 16, -1, 6, 7):
            assert call(K=K) == EINVAL, (call.__name__, K)
        assert call(ld=2) == EINVAL
        assert call(C=0, ld=3) == EINVAL and call(C=-1, ld=3) == EINVAL
        assert call(H=7) == EINVAL and call(W=7) == EINVAL and call(H=7, W=7) == EINVAL       # an image smaller than the tile


# ---------------------------------------------------------------------------------------------- 2. window tables and names
def test_window_tables():
    from patchgan_amd.engine import window_table
    assert window_table('pyramid', 8).tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and window_table('pyramid', 8).dtype == np.float64
    assert window_table('pyramid', 7).tolist() == [1, 2, 3, 4, 3, 2, 1]
    for size in (7, 8, 256):
        h = window_table('hann', size)
        assert h.dtype == np.float64 and np.array_equal(h, np.sin(np.pi * (np.arange(size) + 0.5) / size) ** 2) and (h > 0).all()
        assert np.array_equal(window_table(None, size), np.ones(size))
    custom = [0.5, 1, 2, 3, 3, 2, 1, 0.25]
    assert window_table(custom, 8).tolist() == custom and window_table(tuple(custom), 8).dtype == np.float64
    assert np.array_equal(window_table(np.float32(custom), 8), np.float64(custom))


@pytest.mark.parametrize('bad', [0.0, -1.0, float('nan'), float('inf'), -float('inf')], ids=str)
def test_window_entries_must_be_finite_and_positive(bad):
    from patchgan_amd.engine import window_table
    table = [1.0] * 8
    table[3] = bad
    with pytest.raises(ValueError):
        window_table(table, 8)


def test_window_and_tta_names_and_lengths():
    from patchgan_amd.engine import tta_variants, window_table
    from patchgan_amd.infer import build_mask, n_crop
    for table in ([1.0] * 7, [1.0] * 9, [], [[1.0] * 8]):
        with pytest.raises(ValueError):
            window_table(table, 8)
    for name in ('gauss', 'Hann', ''):
        with pytest.raises(ValueError):
            window_table(name, 8)
    assert [tta_variants(t) for t in (None, 'hflip', 'flips', 'd4')] == [1, 2, 4, 8]
    for name in ('rot90', 'D4', '', 8, ['d4']):
        with pytest.raises(ValueError):
            tta_variants(name)
    with pytest.raises(ValueError):
        n_crop(torch.zeros(3, 13, 19), 8, 0.75, tta='rot90')
    with pytest.raises(ValueError):
        build_mask(torch.zeros(12, 1, 8, 8), 8, (13, 19), 0.5, 0.75, tta='rot90')
    with pytest.raises(ValueError):
        build_mask(torch.zeros(12, 1, 8, 8), 8, (13, 19), 0.5, 0.75, window='gauss')


def test_alias_exports_the_same_functions():
    import patchgan.infer as alias
    import patchgan_amd.infer as I
    assert alias.predict_image is I.predict_image and alias.n_crop is I.n_crop and alias.build_mask is I.build_mask


# ---------------------------------------------------------------------------------------------- 3. host restatement on CPU tensors
def _image(shape):
    c, h, w = shape[:3]
    return torch.rand(c, h, w, generator=torch.Generator().manual_seed(17))


@pytest.mark.parametrize('shape', U.SHAPES, ids=lambda s: f'size{s[3]}')
@pytest.mark.parametrize('K', [1, 2, 4, 8])
def test_n_crop_variants_are_the_torch_ops(shape, K):
    from patchgan_amd.infer import n_crop
    c, h, w, size, overlap = shape
    eff = int(overlap * size)
    assert eff == {8: 6, 7: 5}[size]
    if size == 8:
        assert U.starts(h, size, eff) == [0, 5, 5] and U.starts(w, size, eff) == [0, 6, 11, 11]
    img = _image(shape)
    base = n_crop(img, size, overlap)
    T = base.shape[0]
    assert T == len(U.starts(h, size, eff)) * len(U.starts(w, size, eff))
    got = n_crop(img, size, overlap, tta=U.TTA_NAME[K])
    assert got.shape == (K * T, c, size, size) and got.dtype == base.dtype
    for k in range(K):
        want = base
        if k & 4:
            want = want.transpose(-1, -2)
        if k & 2:
            want = want.flip(-2)
        if k & 1:
            want = want.flip(-1)
        assert torch.equal(got[k * T:(k + 1) * T], want), k
    assert np.array_equal(got.numpy(), U.crops_ref(img.numpy(), size, overlap, K))


@pytest.mark.parametrize('shape', U.SHAPES, ids=lambda s: f'size{s[3]}')
@pytest.mark.parametrize('window', [None, 'pyramid', 'hann'], ids=str)
@pytest.mark.parametrize('K', [1, 2, 4, 8])
@pytest.mark.parametrize('C,thr', [(1, 0.5), (3, 0.0)], ids=['1ch_thr', '3ch_argmax'])
def test_build_mask_equals_the_numpy_loop(shape, window, K, C, thr):
    from patchgan_amd.infer import build_mask
    _, h, w, size, overlap = shape
    eff = int(overlap * size)
    T = len(U.starts(h, size, eff)) * len(U.starts(w, size, eff))
    pred = torch.rand(K * T, C, size, size, generator=torch.Generator().manual_seed(100 + K))
    got = build_mask(pred, size, (h, w), thr, overlap, tta=U.TTA_NAME[K], window=window)
    avg, want = U.blend_ref(pred.numpy(), size, (h, w), overlap, K, U.window(window, size), thr)
    assert got.dtype == want.dtype and got.shape == want.shape == (h, w)
    assert np.array_equal(got, want)
    # the average itself, before threshold / argmax, bit for bit
    got_avg = build_mask(pred[:, :1], size, (h, w), 0, overlap, tta=U.TTA_NAME[K], window=window)
    assert np.array_equal(got_avg, avg[0])
    assert 0.02 < float((want > 0).mean()) < 0.98 or C > 1          # the threshold case is not one-sided


def test_defaults_are_the_unchanged_functions():
    from patchgan_amd.infer import build_mask, n_crop
    c, h, w, size, overlap = U.SHAPES[0]
    img = _image(U.SHAPES[0])
    crops = n_crop(img, size, overlap, tta=None)
    assert torch.equal(crops, n_crop(img, size, overlap)) and np.array_equal(crops.numpy(), U.crops_ref(img.numpy(), size, overlap, 1))
    for C, thr in ((1, 0.5), (3, 0.0)):
        pred = torch.rand(crops.shape[0], C, size, size, generator=torch.Generator().manual_seed(4))
        a = build_mask(pred, size, (h, w), thr, overlap)
        b = build_mask(pred, size, (h, w), thr, overlap, tta=None, window=None)
        assert a.dtype == b.dtype and np.array_equal(a, b)
        assert np.array_equal(a, U.blend_ref(pred.numpy(), size, (h, w), overlap, 1, np.ones(size), thr)[1])
        # a window of ones is the uniform average, bit for bit
        assert np.array_equal(a, build_mask(pred, size, (h, w), thr, overlap, window=[1.0] * size))
