"""Test-time augmentation and windowed blend on the GPU: pg_tiles_gather_tta / pg_tiles_blend_win against torch ops and the plain-NumPy
loops of tests/tta_util.py (bit for bit: the kernel fixes the order and rounding of every double operation), containment in guarded
buffers, the reduction to pg_tiles_blend, predict_image end to end and the patchgan_infer YAML keys.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import tta_util as U

pytestmark = pytest.mark.gpu

PG_OK = 0
KS = [1, 2, 4, 8]
CUSTOM = {8: [0.5, 1.0, 2.0, 3.0, 3.0, 2.0, 1.0, 0.25], 7: [0.3, 1.0, 1.7, 2.9, 1.7, 1.0, 0.1]}
ids_shape = dict(ids=lambda s: f'size{s[3]}')


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _dyadic(*shape, seed):
    """multiples of 2^-8 in [0, 1]"""
    return torch.randint(0, 257, shape, generator=torch.Generator().manual_seed(seed)).float() / 256


def _ntiles(shape):
    _, h, w, size, overlap = shape
    eff = int(overlap * size)
    return len(U.starts(h, size, eff)) * len(U.starts(w, size, eff))


def _blend_both(pred, shape, K, table, thr):
    """pg_tiles_blend_win with both outputs, predictions in a strided view: (mask [C, H, W] float64, argmax [H, W] int64) as numpy"""
    from patchgan_amd import engine as E
    _, h, w, size, overlap = shape
    n, c = pred.shape[:2]
    pv = E.View.alloc(n, size, size, c + 1, 'cuda').channels(1, c).from_nchw(pred.cuda())
    win = torch.as_tensor(np.asarray(table, dtype=np.float64)).cuda()
    mask = torch.empty(c, h, w, dtype=torch.float64, device='cuda')
    arg = torch.empty(h, w, dtype=torch.int64, device='cuda')
    rc = _lib().pg_tiles_blend_win(pv.ptr(), pv.ld, c, size, int(overlap * size), h, w, K, win.data_ptr(), float(thr), mask.data_ptr(),
                                   arg.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    return mask.cpu().numpy(), arg.cpu().numpy()


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize('shape', U.SHAPES, **ids_shape)
def test_gather_variants_are_the_torch_ops(shape):
    from patchgan_amd import engine as E
    from tests import guard_util as G
    c, h, w, size, overlap = shape
    img = torch.rand(c, h, w, generator=torch.Generator().manual_seed(17)).cuda()
    base = E.tiles_gather(img, size, overlap).to_nchw()
    T = _ntiles(shape)
    assert base.shape[0] == T
    for K in KS:
        v = E.tiles_gather(img, size, overlap, tta=U.TTA_NAME[K])
        assert (v.N, v.H, v.W, v.C) == (K * T, size, size, c)
        got = v.to_nchw()
        assert np.array_equal(got.cpu().numpy(), U.crops_ref(img.cpu().numpy(), size, overlap, K))
        for k in range(K):
            want = base
            if k & 4:
                want = want.transpose(-1, -2)
            if k & 2:
                want = want.flip(-2)
            if k & 1:
                want = want.flip(-1)
            assert torch.equal(got[k * T:(k + 1) * T], want), (K, k)
        # into a channel slice of a wider buffer: nothing outside the slice is written
        ins = G.Inputs()
        gi = ins.add(G.flat_from(img), 'image')
        vt, gt = G.view(K * T, size, size, c, ld=c + 2, off=1)
        assert _lib().pg_tiles_gather_tta(gi.ptr(), c, h, w, size, int(overlap * size), K, vt.ptr(), vt.ld, None) == PG_OK
        torch.cuda.synchronize()
        G.assert_untouched(gt, 'slice', f'tiles_gather_tta K={K}')
        assert torch.equal(G.read_nchw(vt).float(), got)
        ins.check(f'tiles_gather_tta K={K}')


# ---------------------------------------------------------------------------------------------- blend, exact arithmetic
@pytest.mark.parametrize('shape', U.SHAPES, **ids_shape)
@pytest.mark.parametrize('K', KS)
def test_blend_exact_on_dyadic_predictions(shape, K):
    """Predictions k / 256 and integer pyramid weights <= 4 * 4: every product and every sum of at most 9 * 8 terms is exact in double,
    so the only rounding is the final division."""
    c, h, w, size, overlap = shape
    pred = _dyadic(K * _ntiles(shape), c, size, size, seed=30 + K)
    win = U.window('pyramid', size)
    for thr in (0.0, 0.5):
        avg, want_arg = U.blend_ref(pred.numpy(), size, (h, w), overlap, K, win, thr)
        mask, arg = _blend_both(pred, shape, K, win, thr)
        want_mask = (avg >= thr).astype(np.float64) if thr > 0 else avg
        assert np.array_equal(mask, want_mask), (thr, np.abs(mask - want_mask).max())
        assert np.array_equal(arg, want_arg), thr
    # through the engine: one channel returns the mask, several the argmax
    from patchgan_amd import engine as E
    for ch, thr in ((1, 0.5), (c, 0.0)):
        pv = E.View.alloc(pred.shape[0], size, size, ch, 'cuda').from_nchw(pred[:, :ch].contiguous().cuda())
        got = E.tiles_blend(pv, (h, w), thr, overlap, tta=U.TTA_NAME[K], window='pyramid').cpu().numpy()
        want = U.blend_ref(pred[:, :ch].numpy(), size, (h, w), overlap, K, win, thr)[1]
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize('shape', U.SHAPES, **ids_shape)
@pytest.mark.parametrize('window', ['pyramid', None], ids=str)
def test_identity_model_returns_the_image(shape, window):
    """gather with K = 8, take the tiles as the predictions, blend: every term of a pixel is the same dyadic value, so the weighted
    average is that value exactly."""
    from patchgan_amd import engine as E
    c, h, w, size, overlap = shape
    img = _dyadic(c, h, w, seed=5)
    tiles = E.tiles_gather(img.cuda(), size, overlap, tta='d4')
    one = E.tiles_gather(img[:1].cuda(), size, overlap, tta='d4')
    assert np.array_equal(E.tiles_blend(one, (h, w), 0, overlap, tta='d4', window=window).cpu().numpy(), img[0].double().numpy())
    assert np.array_equal(E.tiles_blend(tiles, (h, w), 0, overlap, tta='d4', window=window).cpu().numpy(), np.argmax(img.numpy(), axis=0))
    mask, _ = _blend_both(tiles.to_nchw().cpu(), shape, 8, U.window(window, size), 0.0)
    assert np.array_equal(mask, img.double().numpy())


# ---------------------------------------------------------------------------------------------- blend, general values
@pytest.mark.parametrize('shape', U.SHAPES, **ids_shape)
@pytest.mark.parametrize('window', ['hann', 'custom'])
@pytest.mark.parametrize('K', KS)
def test_blend_general_equals_the_numpy_loop(shape, window, K):
    """torch.rand predictions under irrational / uneven weights: equal bit for bit because the kernel does the NumPy loop's IEEE
    operations in its order, none contracted."""
    c, h, w, size, overlap = shape
    pred = torch.rand(K * _ntiles(shape), c, size, size, generator=torch.Generator().manual_seed(60 + K))
    table = U.window('hann', size) if window == 'hann' else np.float64(CUSTOM[size])
    for thr in (0.0, 0.5):
        avg, want_arg = U.blend_ref(pred.numpy(), size, (h, w), overlap, K, table, thr)
        mask, arg = _blend_both(pred, shape, K, table, thr)
        want_mask = (avg >= thr).astype(np.float64) if thr > 0 else avg
        print(f'K={K} {window} thr={thr}: max |kernel - numpy| = {np.abs(mask - want_mask).max():.3e}')
        assert np.array_equal(mask, want_mask)
        assert np.array_equal(arg, want_arg)
    # the engine takes the table as a name or as a sequence
    from patchgan_amd import engine as E
    pv = E.View.alloc(pred.shape[0], size, size, 1, 'cuda').from_nchw(pred[:, :1].contiguous().cuda())
    got = E.tiles_blend(pv, (h, w), 0, overlap, tta=U.TTA_NAME[K], window='hann' if window == 'hann' else CUSTOM[size])
    assert np.array_equal(got.cpu().numpy(), U.blend_ref(pred[:, :1].numpy(), size, (h, w), overlap, K, table, 0)[1])


def test_ones_window_single_variant_is_the_old_kernel():
    """pg_tiles_blend_win with a table of ones and K = 1 against pg_tiles_blend on random data, at the non-square 2 x 600 x 1024 case."""
    lib = _lib()
    C, H, W, size, eff = 2, 600, 1024, 256, int(0.9 * 256)
    T = lib.pg_tiles_count(H, size, eff) * lib.pg_tiles_count(W, size, eff)
    assert T == 15
    gen = torch.Generator(device='cuda').manual_seed(9)
    pred = torch.rand(T * size * size * (C + 1), device='cuda', generator=gen)          # NHWC, ld = C + 1, slice at offset 1
    ones = torch.ones(size, dtype=torch.float64, device='cuda')
    for thr in (0.0, 0.5):
        out = []
        for new in (False, True):
            mask = torch.empty(C, H, W, dtype=torch.float64, device='cuda')
            arg = torch.empty(H, W, dtype=torch.int64, device='cuda')
            if new:
                rc = lib.pg_tiles_blend_win(pred.data_ptr() + 4, C + 1, C, size, eff, H, W, 1, ones.data_ptr(), thr, mask.data_ptr(),
                                            arg.data_ptr(), None)
            else:
                rc = lib.pg_tiles_blend(pred.data_ptr() + 4, C + 1, C, size, eff, H, W, thr, mask.data_ptr(), arg.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == PG_OK
            out.append((mask, arg))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), thr
        assert 0 < int(out[0][1].sum()) < H * W


# ---------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize('shape', U.SHAPES, **ids_shape)
def test_blend_win_containment(shape):
    """mask of exactly C*H*W doubles, argmax of exactly H*W int64, each alone and both together; the predictions (a channel slice) and
    the window table are not written."""
    from tests import guard_util as G
    lib = _lib()
    c, h, w, size, overlap = shape
    eff, K = int(overlap * size), 8
    pred = torch.rand(K * _ntiles(shape), c, size, size, generator=torch.Generator().manual_seed(2))
    table = U.window('hann', size)
    ins = G.Inputs()
    vt, gt = G.view_from(pred, ld=c + 2, off=1)
    ins.add(gt, 'tiles')
    gw = ins.add(G.flat_from(torch.as_tensor(table)), 'window')
    avg, want_arg = U.blend_ref(pred.numpy(), size, (h, w), overlap, K, table, 0.0)
    for with_mask, with_arg in ((True, False), (False, True), (True, True)):
        mask = G.flat(c * h * w * 8) if with_mask else None
        arg = G.flat(h * w * 8) if with_arg else None
        rc = lib.pg_tiles_blend_win(vt.ptr(), vt.ld, c, size, eff, h, w, K, gw.ptr(), 0.0, mask.ptr() if mask else None,
                                    arg.ptr() if arg else None, None)
        torch.cuda.synchronize()
        assert rc == PG_OK
        if mask:
            G.assert_untouched(mask, 'all', 'tiles_blend_win mask')
            assert np.array_equal(mask.inner(torch.float64).view(c, h, w).cpu().numpy(), avg)
        if arg:
            G.assert_untouched(arg, 'all', 'tiles_blend_win argmax')
            assert np.array_equal(arg.inner(torch.int64).view(h, w).cpu().numpy(), want_arg)
    ins.check('tiles_blend_win')


def test_engine_refuses_what_does_not_fit():
    from patchgan_amd import engine as E
    img = torch.rand(3, 13, 19).cuda()
    tiles = E.tiles_gather(img, 8, 0.75, tta='flips')
    with pytest.raises(ValueError):
        E.tiles_blend(tiles, (13, 19), 0, 0.75, tta='d4')           # 4 variants are not 8
    with pytest.raises(ValueError):
        E.tiles_blend(tiles, (13, 19), 0, 0.75)
    with pytest.raises(ValueError):
        E.tiles_blend(tiles, (13, 19), 0, 0.75, tta='flips', window=[1.0] * 7)
    with pytest.raises(ValueError):
        E.tiles_gather(img, 8, 0.75, tta='rot90')
    with pytest.raises(ValueError):
        E.tiles_gather(torch.rand(3, 7, 19).cuda(), 8, 0.75, tta='d4')
    # the table is uploaded once per (window, size, device)
    a = E.window_dev('hann', 8, 'cuda')
    assert E.window_dev('hann', 8, torch.device('cuda', torch.cuda.current_device())) is a
    assert E.window_dev([1.0, 2.0], 2, 'cuda') is E.window_dev((1.0, 2.0), 2, 'cuda')
    assert E.window_dev('hann', 7, 'cuda') is not a


# ---------------------------------------------------------------------------------------------- end to end
def _generator(kind):
    import patchgan_amd as pg
    from torch import nn
    torch.manual_seed(11)
    if kind == 'bn128':
        g = pg.UNet(3, 1, 4, norm_layer=nn.BatchNorm2d, final_act='sigmoid')
        return g.cuda().eval(), 128, (160, 200), 0.5
    g = pg.UNet(3, 3, 4, final_act='softmax')
    return g.cuda().eval(), 256, (300, 300), 0.0


@pytest.mark.parametrize('kind', ['bn128', 'in256'])
def test_predict_image_equals_ncrop_forward_build_mask(kind):
    """predict_image (gather -> generator -> blend, NHWC throughout) with d4 and the pyramid window equals the host composition
    n_crop -> generator(NCHW) -> build_mask bit for bit: the module forward gets the same K * T batch in the same order."""
    from patchgan_amd.infer import build_mask, n_crop, predict_image
    g, size, (h, w), thr = _generator(kind)
    img = torch.rand(3, h, w, generator=torch.Generator().manual_seed(5)).cuda()
    crops = n_crop(img, size, 0.9, tta='d4')
    assert crops.shape[0] == 8 * 4
    got = predict_image(g, img, size, 0.9, thr, max_tiles=crops.shape[0], tta='d4', window='pyramid')
    with torch.no_grad():
        masks = g(crops)
    want = build_mask(masks, size, (h, w), thr, 0.9, tta='d4', window='pyramid')
    assert got.dtype == want.dtype and got.shape == want.shape == (h, w)
    np.testing.assert_array_equal(got, want)
    if thr == 0 and got.dtype == np.float64:
        assert np.ptp(got) > 0
    # both None: today's call, today's result
    base = predict_image(g, img, size, 0.9, thr)
    np.testing.assert_array_equal(predict_image(g, img, size, 0.9, thr, tta=None, window=None), base)
    with torch.no_grad():
        np.testing.assert_array_equal(base, build_mask(g(n_crop(img, size, 0.9)), size, (h, w), thr, 0.9))
    # a bad argument is refused before any launch
    with pytest.raises(ValueError):
        predict_image(g, img, size, 0.9, thr, tta='rot90')
    with pytest.raises(ValueError):
        predict_image(g, img, size, 0.9, thr, window=[0.0] * size)


# ---------------------------------------------------------------------------------------------- CLI
PLUGIN = '''
import os
import numpy as np
import torch
from torch.utils.data import Dataset


class Noise(Dataset):
    """two 3 x 300 x 300 noise images: four 256-pixel tiles each"""
    def __init__(self, path, **kw):
        self.n = 2

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if i >= self.n:
            raise IndexError
        return torch.rand(3, 300, 300, generator=torch.Generator().manual_seed(40 + i))

    def get_filename(self, i):
        return f'noise_{i:03d}.png'

    @staticmethod
    def save_mask(mask, out_dir, fname):
        np.save(os.path.join(out_dir, fname + '.npy'), mask)
'''


def test_cli_reads_tta_and_window(tmp_path, monkeypatch):
    import patchgan_amd as pg
    from patchgan_amd.infer import patchgan_infer, predict_image
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    torch.manual_seed(21)
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    torch.save(g.state_dict(), tmp_path / 'g.pth')
    torch.save(d.state_dict(), tmp_path / 'd.pth')
    g.cuda().eval()
    imgs = [torch.rand(3, 300, 300, generator=torch.Generator().manual_seed(40 + i)).cuda() for i in range(2)]
    masks = {}
    for tag, extra in (('plain', {}), ('tta', {'tta': 'hflip', 'window': 'hann'})):
        cfg = {'dataset': {'type': 'Noise', 'dataset_path': 'unused', 'size': 256},
               'model_params': {'gen_filts': 4, 'disc_filts': 4, 'n_disc_layers': 3, 'activation': 'leakyrelu'},
               'checkpoint_paths': {'generator': str(tmp_path / 'g.pth'), 'discriminator': str(tmp_path / 'd.pth')},
               'infer_params': dict({'output_path': str(tmp_path / tag)}, **extra)}
        (tmp_path / f'{tag}.yaml').write_text(yaml.safe_dump(cfg))
        patchgan_infer(['-c', f'{tag}.yaml'])
        for i, img in enumerate(imgs):
            saved = np.load(tmp_path / tag / f'noise_{i:03d}.npy')
            want = predict_image(g, img, 256, 0.9, 0, **extra)
            assert saved.shape == (300, 300) and saved.dtype == want.dtype
            np.testing.assert_array_equal(saved, want)
            masks[tag, i] = saved
    assert not np.array_equal(masks['plain', 0], masks['tta', 0])          # the keys reach the kernels
    # the window as a list
    table = [float(min(u + 1, 256 - u)) for u in range(256)]
    cfg['infer_params'] = {'output_path': str(tmp_path / 'listed'), 'window': table}
    (tmp_path / 'listed.yaml').write_text(yaml.safe_dump(cfg))
    patchgan_infer(['-c', 'listed.yaml'])
    np.testing.assert_array_equal(np.load(tmp_path / 'listed' / 'noise_001.npy'), predict_image(g, imgs[1], 256, 0.9, 0, window='pyramid'))
