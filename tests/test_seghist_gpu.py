"""Score curves on the GPU: pg_seg_hist against the NumPy statement of its rule, exactly (A), views, accumulation, containment and
stream (B), the trainer's evaluation steps, evaluate() and train() (C), the command-line tools with `threshold: best` (D), two
data-parallel ranks (E).  Integer counts: every comparison is np.array_equal.  Needs an MI355X."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from tests.golden_util import LOSS_KEYS
from tests.metrics_util import confusion_ref, make_case
from tests.seghist_util import edge_case, hist_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(3, 5, 5), (2, 33, 31), (3, 256, 256)]      # 75 pixels: part of one workgroup; 2046: a ragged tail; 196608: a second trip
SHAPE_IDS = ['75px', '2046px', '196608px']
_CASES, _REFS = {}, {}


def _case(N, C, H, W, kind='eighths'):
    """One (p, y) per shape and kind, made once and shared (never modified).  'eighths' / 'soft': metrics_util.make_case (predictions
    are multiples of 1/8: on bin borders); 'uniform': random float32 predictions in [0, 1); 'saturated': every prediction 0 or 1."""
    key = (N, C, H, W, kind)
    if key not in _CASES:
        seed = 2000 + 31 * C + N * H
        p, y = make_case(N, C, H, W, seed=seed + (7 if kind == 'soft' else 0), soft=kind == 'soft')
        rng = np.random.default_rng(seed + 1)
        if kind == 'uniform':
            p = rng.random((N, C, H, W), dtype=np.float32)
        elif kind == 'saturated':
            p = (rng.random((N, C, H, W)) > 0.6).astype(np.float32)
        _CASES[key] = (p, y)
    return _CASES[key]


def _ref(p, y, bins):
    """hist_ref of a shared case, computed once."""
    key = (id(p), id(y), bins)
    if key not in _REFS:
        _REFS[key] = (p, y) + hist_ref(p, y, bins)          # (p and y are kept alive: their ids stay theirs)
    return _REFS[key][2:]


def _table(C, bins, fill=None):
    t = torch.zeros(C * 2 * bins + 1, dtype=torch.int64, device=DEV)
    if fill is not None:
        t += fill.to(DEV)
    return t


def _split(a, C, bins):
    n = C * 2 * bins
    return a[:n].reshape(C, 2, bins), int(a[n])


def _run(p, y, bins, ld_p=None, off_p=0, ld_y=None, off_y=0, hist=None):
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view
    C = p.shape[1]
    pv = to_view(torch.from_numpy(p), ld_p, off_p)
    yv = to_view(torch.from_numpy(y), ld_y, off_y)
    hist = _table(C, bins) if hist is None else hist
    E.seg_hist(pv, yv, bins, hist)
    return _split(hist.cpu().numpy(), C, bins)


def _check(p, y, bins, **views):
    hist, ign = _run(p, y, bins, **views)
    want, want_ign = _ref(p, y, bins)
    assert hist.dtype == np.int64 and np.array_equal(hist, want), np.argwhere(hist != want)[:8]
    assert ign == want_ign
    N, C, H, W = p.shape
    assert hist.sum() + ign == C * (N * H * W - ign) + ign          # every kept pixel adds exactly one count per channel
    return hist, ign


# ---------------------------------------------------------------------------------------------- A. exactness
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('C', [1, 2, 3, 4, 7, 32])
def test_table_equals_numpy_at_16_bins(C, shape):
    N, H, W = shape
    hist, ign = _check(*_case(N, C, H, W), 16)
    if shape == SHAPES[2]:
        assert (ign > 0) == (C > 1) and (hist[:, :, ::2] > 0).all()          # the data reaches both labels of every channel


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('C,bins', [(1, 256), (1, 1024), (4, 256), (32, 256)], ids=['c1_b256', 'c1_b1024', 'c4_b256', 'c32_b256_64KiB'])
def test_table_equals_numpy_on_random_predictions(C, bins, shape):
    N, H, W = shape
    hist, _ = _check(*_case(N, C, H, W, 'uniform'), bins)
    if shape == SHAPES[2] and C * bins <= 1024:
        assert np.count_nonzero(hist) > 0.9 * hist.size          # the bins in between are used


@pytest.mark.parametrize('C,bins,kind', [(1, 16, 'eighths'), (1, 256, 'saturated'), (4, 16, 'eighths'), (4, 256, 'uniform')])
def test_three_trips_of_256_workgroups(C, bins, kind):
    """327680 pixels: the grid's largest, 256 workgroups of 512, covers 131072 per trip -- a third, ragged trip on the one- and
    four-channel paths (the 64-KiB table above gets 32 workgroups and takes twelve trips for 196608 pixels)."""
    _check(*_case(5, C, 256, 256, kind), bins)


@pytest.mark.parametrize('C,bins', [(1, 16), (1, 256), (1, 1024), (4, 16), (4, 256)])
def test_edge_values(C, bins):
    """Every k / bins with its neighbours one ulp to either side, a denormal, -0.0, values outside [0, 1]."""
    p, y = edge_case(C, bins, seed=40 + C + bins)
    hist, ign = _run(p, y, bins)
    want, want_ign = hist_ref(p, y, bins)
    assert np.array_equal(hist, want) and ign == want_ign


@pytest.mark.parametrize('shape', SHAPES[1:], ids=SHAPE_IDS[1:])
@pytest.mark.parametrize('C,bins', [(1, 16), (1, 256), (4, 256), (3, 16)])
def test_saturated_predictions(C, bins, shape):
    """Every prediction is 0 or 1: whole waves land on the first and last bin of one label."""
    N, H, W = shape
    p, y = _case(N, C, H, W, 'saturated')
    hist, ign = _check(p, y, bins)
    assert hist[:, :, 1:-1].sum() == 0 and (hist[:, :, 0] > 0).all() and (hist[:, :, -1] > 0).all()
    if C == 1:
        ones = np.ones_like(p)
        got, _ = _run(ones, y, bins)
        assert got[0, 1, -1] == (y >= 0.5).sum() and got[0, 0, -1] == (y < 0.5).sum() and got.sum() == p.size


@pytest.mark.parametrize('C', [2, 4, 7])
def test_soft_targets_take_their_argmax(C):
    N, H, W = SHAPES[1]
    p, y = _case(N, C, H, W, 'soft')
    assert ((y > 0) & (y < 1)).any()
    _check(p, y, 16)
    _check(p, y, 16, ld_p=C + 3, off_p=3, ld_y=C + 3, off_y=3)


# ---------------------------------------------------------------------------------------------- B. views, buffers, streams
VIEWS = {
    'c4_vector_ld4': (4, dict(ld_p=4, ld_y=4)),                                  # 16-byte loads
    'c4_off3_ld7': (4, dict(ld_p=7, off_p=3, ld_y=7, off_y=3)),                  # the discriminator-input layout: by element
    'c4_off4_ld8': (4, dict(ld_p=8, off_p=4, ld_y=8, off_y=4)),                  # aligned slice of 8-float pixels
    'c4_off2_ld8': (4, dict(ld_p=8, off_p=2, ld_y=8, off_y=2)),                  # ld a multiple of 4, the offset not: leaves the 16-byte path
    'c4_mixed': (4, dict(ld_p=4, ld_y=7, off_y=3)),                              # one operand by vector, the other by element
    'c1_off3_ld4': (1, dict(ld_p=4, off_p=3, ld_y=4, off_y=3)),
    'c3_off2_ld6': (3, dict(ld_p=6, off_p=2, ld_y=5, off_y=1)),
}


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('name', list(VIEWS))
def test_table_equals_numpy_on_channel_slices(name, shape):
    """The other channels of the wider pixels are NaN (gpu_util.to_view): a result that equals the reference did not read them."""
    C, views = VIEWS[name]
    N, H, W = shape
    _check(*_case(N, C, H, W), 16, **views)
    _check(*_case(N, C, H, W, 'uniform'), 256, **views)


@pytest.mark.parametrize('C', [1, 4])
def test_two_launches_add_to_what_the_buffer_holds(C):
    bins = 16
    p1, y1 = _case(*SHAPES[1][:1], C, *SHAPES[1][1:])
    p2, y2 = _case(*SHAPES[2][:1], C, *SHAPES[2][1:])
    # counts already there, the first next to a carry out of the low 32 bits
    before = torch.arange(C * 2 * bins + 1, dtype=torch.int64) * 1000 + 5
    before[0] = (1 << 32) - 3
    hist = _table(C, bins, before)
    _run(p1, y1, bins, hist=hist)
    got, ign = _run(p2, y2, bins, hist=hist)
    r1, r2 = _ref(p1, y1, bins), _ref(p2, y2, bins)
    b, bi = _split(before.numpy(), C, bins)
    assert r1[0][0, 0, 0] + r2[0][0, 0, 0] > 3          # (the carry happens)
    assert np.array_equal(got, b + r1[0] + r2[0])
    assert ign == bi + r1[1] + r2[1]


@pytest.mark.parametrize('name', ['c4_off3_ld7', 'c4_off4_ld8', 'c1_off3_ld4', 'c3_off2_ld6', 'c4_vector_ld4'])
def test_containment(name):
    """p and y in guarded views whose other channels are the 0xFF sentinel (NaN), the table in a guarded flat buffer: the inputs stay
    byte-identical, only the C*2*bins + 1 words change, and the table equals the reference (the neighbours were not read into it)."""
    from tests import guard_util as G
    from patchgan_amd import _lib as L
    C, v = VIEWS[name]
    bins = 16
    N, H, W = SHAPES[1]
    p, y = _case(N, C, H, W)
    pv, pg_ = G.view_from(torch.from_numpy(p), v.get('ld_p'), v.get('off_p', 0))
    yv, yg = G.view_from(torch.from_numpy(y), v.get('ld_y'), v.get('off_y', 0))
    hg = G.flat((C * 2 * bins + 1) * 8)
    hg.inner(torch.int64).zero_()
    ins = G.Inputs()
    ins.add(pg_, 'p')
    ins.add(yg, 'y')
    torch.cuda.synchronize()
    rc = L.load().pg_seg_hist(pv.ptr(), pv.ld, yv.ptr(), yv.ld, N, H * W, C, bins, hg.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    G.assert_untouched(hg, 'all', 'seg_hist table')
    ins.check('seg_hist')
    got, ign = _split(hg.inner(torch.int64).cpu().numpy(), C, bins)
    want, want_ign = _ref(p, y, bins)
    assert np.array_equal(got, want) and ign == want_ign


def test_launch_goes_to_the_current_stream():
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view
    N, H, W = SHAPES[2]
    p, y = _case(N, 4, H, W)
    pv, yv = to_view(torch.from_numpy(p), 7, 3), to_view(torch.from_numpy(y), 7, 3)
    hist = _table(4, 16)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        E.seg_hist(pv, yv, 16, hist)
        host = torch.empty(4 * 2 * 16 + 1, dtype=torch.int64).pin_memory()
        host.copy_(hist, non_blocking=True)
    s.synchronize()
    got, ign = _split(host.numpy(), 4, 16)
    want, want_ign = _ref(p, y, 16)
    assert np.array_equal(got, want) and ign == want_ign


# ---------------------------------------------------------------------------------------------- C. trainer
def _nets(cout, seed=11):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, cout, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid' if cout == 1 else 'softmax')
    d = pg.Discriminator(3 + cout, 4, n_layers=3)
    return g.to(DEV), d.to(DEV)


def _trainer(folder, cout, seed=11, **settings):
    import patchgan_amd as pg
    g, d = _nets(cout, seed)
    t = pg.Trainer(g, d, str(folder))
    for k, v in settings.items():
        setattr(t, k, v)
    return t


_BATCHES = {}


def _batches(cout, n=4):
    """n batches (x, y) of two 256 x 256 samples; masks with about 10 % unlabelled pixels where there are several classes."""
    if cout not in _BATCHES:
        gen = torch.Generator().manual_seed(70 + cout)
        out = []
        for _ in range(n):
            x = torch.rand(2, 3, 256, 256, generator=gen)
            if cout == 1:
                y = (torch.rand(2, 1, 256, 256, generator=gen) > 0.7).float()
            else:
                lab = torch.randint(0, cout, (2, 256, 256), generator=gen)
                y = torch.nn.functional.one_hot(lab, cout).permute(0, 3, 1, 2).float()
                y = y * (torch.rand(2, 1, 256, 256, generator=gen) >= 0.1).float()
            out.append((x, y.contiguous()))
        _BATCHES[cout] = out
    return _BATCHES[cout]


def _seg(step_losses):
    step_losses._event.synchronize()
    return float(step_losses._host[0])


CURVE_KEYS = ('curve', 'ap', 'best_threshold', 'best_iou', 'best_dice', 'mean_ap', 'best_miou', 'hist')


@pytest.mark.parametrize('two', [False, True], ids=['one_stream', 'two_streams'])
@pytest.mark.parametrize('cout', [1, 4])
def test_evaluation_step_histograms_its_own_prediction(tmp_path, cout, two):
    bins = 64
    t = _trainer(tmp_path, cout, metrics=True, metric_bins=bins, two_streams=two)
    t.generator.eval()
    t.discriminator.eval()
    x, y = _batches(cout)[0]
    t.batch(x, y, train=False)
    assert t.launch_mode == ('eager2' if two else 'eager1')
    m = t.read_metrics()
    pred = t._last_gen.to_nchw().cpu().numpy()
    want, want_ign = hist_ref(pred, y.numpy(), bins)
    assert m['hist'].shape == (cout, 2, bins) and np.array_equal(m['hist'], want) and m['ignored'] == want_ign
    for k in CURVE_KEYS + ('iou', 'miou', 'confusion'):
        assert k in m, k
    assert m['curve']['iou'].shape == (cout, bins) and m['best_threshold'].shape == (cout,)
    # a second batch adds; reset_metrics() zeroes both tables
    x2, y2 = _batches(cout)[1]
    t.batch(x2, y2, train=False)
    want2, ign2 = hist_ref(t._last_gen.to_nchw().cpu().numpy(), y2.numpy(), bins)
    m2 = t.read_metrics()
    assert np.array_equal(m2['hist'], want + want2) and m2['ignored'] == want_ign + ign2
    t.reset_metrics()
    m3 = t.read_metrics()
    assert m3['hist'].sum() == 0 and m3['confusion'].sum() == 0


@pytest.mark.parametrize('k', [1, 24, 32, 63])
def test_curve_at_k_equals_the_confusion_counts_at_that_threshold(tmp_path, k):
    bins = 64
    t = _trainer(tmp_path, 1, metrics=True, metric_bins=bins, metric_threshold=k / bins)
    t.generator.eval()
    t.discriminator.eval()
    for x, y in _batches(1)[:2]:
        t.batch(x, y, train=False)
    m = t.read_metrics()
    cv = m['curve']
    got = np.array([[cv['tn'][0, k], cv['fp'][0, k]], [cv['fn'][0, k], cv['tp'][0, k]]])
    assert np.array_equal(got, m['confusion']) and m['confusion'].sum() == 2 * 2 * 256 * 256
    assert cv['iou'][0, k] == m['iou'][1] and cv['dice'][0, k] == m['dice'][1]
    assert cv['precision'][0, k] == m['precision'][1] or (np.isnan(cv['precision'][0, k]) and np.isnan(m['precision'][1]))


@pytest.mark.parametrize('cout', [1, 4])
def test_losses_and_counts_are_bit_identical_with_and_without_metric_bins(tmp_path, cout):
    b = _batches(cout)
    rows, confs = {}, {}
    for bins in (None, 256):
        t = _trainer(tmp_path / str(bins), cout, metrics=True, metric_bins=bins)
        t.setup_optimizers(1e-3, 1e-3)
        t.generator.train()
        t.discriminator.train()
        out = []
        for i, train in enumerate((True, True, False, True)):
            out.append(dict(t.batch(*b[i], train=train)))
            if i < 2 or bins is None:
                assert t.seg_hist is None                       # training steps never touch (or create) the table; off: no buffer
        t.flush()
        m = t.read_metrics()
        assert ('hist' in m) == (bins is not None) and ('curve' in m) == (bins is not None)
        if bins:
            assert m['hist'].sum() + m['ignored'] == cout * (2 * 256 * 256 - m['ignored']) + m['ignored']
        rows[bins], confs[bins] = out, (m['confusion'], m['ignored'])
    assert rows[None] == rows[256]
    assert np.array_equal(confs[None][0], confs[256][0]) and confs[None][1] == confs[256][1]
    assert all(set(r) == set(LOSS_KEYS) for r in rows[256])


def test_metric_bins_without_metrics_raises_at_the_first_evaluation_step(tmp_path):
    t = _trainer(tmp_path, 1, metric_bins=256)
    t.setup_optimizers(1e-3, 1e-3)
    x, y = _batches(1)[0]
    with pytest.raises(ValueError, match='needs Trainer.metrics = True'):
        t.batch(x, y, train=False)
    t.flush()


@pytest.mark.parametrize('cout', [1, 4])
def test_evaluate_equals_evaluation_steps(tmp_path, cout):
    t = _trainer(tmp_path, cout, metrics=True, metric_bins=128)
    t.generator.eval()
    t.discriminator.eval()
    data = _batches(cout)[:2]
    segs = [_seg(t.batch(x, y, train=False)) for x, y in data]
    m = t.read_metrics()
    ev = t.evaluate(data)
    assert np.array_equal(ev['hist'], m['hist']) and np.array_equal(ev['confusion'], m['confusion']) and ev['ignored'] == m['ignored']
    assert ev['seg_loss'] == (segs[0] + segs[1]) / 2
    assert np.array_equal(ev['best_threshold'], m['best_threshold'], equal_nan=True) and np.array_equal(ev['ap'], m['ap'], equal_nan=True)
    assert np.array_equal(t.read_metrics()['hist'], m['hist'])          # a table of its own, not the trainer's
    t.metric_bins = None
    assert 'hist' not in t.evaluate(data) and 'hist' not in t.read_metrics()


def test_evaluate_the_averaged_generator(tmp_path):
    cout, bins = 1, 64
    t = _trainer(tmp_path, cout, ema_decay=0.9, metrics=True, metric_bins=bins)
    t.setup_optimizers(1e-3, 1e-3)
    t.generator.train()
    t.discriminator.train()
    b = _batches(cout)
    for i in range(3):
        t.batch(*b[i], train=True)
    data = b[2:4]
    ev = t.evaluate(data, t.ema_generator)
    live = t.evaluate(data)
    assert ev['hist'].sum() == 2 * 2 * 256 * 256 == live['hist'].sum()
    assert not np.array_equal(ev['hist'], live['hist'])
    k = 32                                                                   # metric_threshold 0.5 = 32 / 64
    cv = ev['curve']
    assert np.array_equal([[cv['tn'][0, k], cv['fp'][0, k]], [cv['fn'][0, k], cv['tp'][0, k]]], ev['confusion'])
    assert t.seg_hist is None                                                # evaluate() does not create the trainer's table


def test_train_writes_the_best_threshold_and_prints_it(tmp_path, capsys):
    t = _trainer(tmp_path / 'on', 1, seed=21, ema_decay=0.9, metrics=True, save_best='miou', metric_bins=64)
    b = _batches(1)
    t.train(b[:2], b[2:4], 2, save_freq=1)
    printed = capsys.readouterr().out
    lines = [ln for ln in printed.splitlines() if ln.startswith('Validation metrics')]
    assert len(lines) == 2 and all(ln.count('mean AP') == 2 and ln.count('best threshold') == 2 and 'with IoU' in ln for ln in lines)
    h = t.val_history
    assert [e['epoch'] for e in h] == [1, 2]
    for e in h:
        for k in ('miou', 'confusion', 'ap', 'best_threshold', 'best_iou', 'best_dice', 'mean_ap', 'best_miou'):
            assert k in e and k in e['ema'], k
        for k in ('curve', 'hist'):
            assert k not in e and k not in e['ema'], k
        assert 1 / 64 <= e['best_threshold'][0] <= 63 / 64
    best = json.load(open(os.path.join(t.savefolder, 'best_metrics.json')))
    for name in ('generator', 'generator_ema'):
        s = best[name]['scores']
        e = h[best[name]['epoch'] - 1]
        e = e if name == 'generator' else e['ema']
        assert s['best_threshold'] == [float(e['best_threshold'][0])] and s['mean_ap'] == e['mean_ap']
        assert 'curve' not in s and 'hist' not in s
        assert best[name]['score'] == e['miou']                              # the criterion stays miou at metric_threshold
    from patchgan_amd.metrics import best_threshold
    assert best_threshold(os.path.join(t.savefolder, 'best_generator.pth'), 1) == best['generator']['scores']['best_threshold'][0]

    # off: the line and the file are the ones without the feature
    t2 = _trainer(tmp_path / 'off', 1, seed=21, ema_decay=0.9, metrics=True, save_best='miou')
    t2.train(b[:2], b[2:4], 1, save_freq=1)
    out = capsys.readouterr().out
    assert 'Validation metrics' in out and 'mean AP' not in out and 'best threshold' not in out
    assert t2.seg_hist is None and 'best_threshold' not in t2.val_history[0]
    assert 'best_threshold' not in json.load(open(os.path.join(t2.savefolder, 'best_metrics.json')))['generator']['scores']


# ---------------------------------------------------------------------------------------------- D. command line
def test_cli_trains_with_metric_bins_and_infers_at_the_best_threshold(tmp_path, monkeypatch, capsys):
    """patchgan_train with metric_bins writes best_threshold; patchgan_infer with `threshold: best` gives, array for array, what it
    gives with that number written out, and refuses an epoch checkpoint."""
    import yaml
    from tests.test_cli_gpu import PLUGIN
    from patchgan_amd.train import patchgan_train
    from patchgan_amd.infer import patchgan_infer
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    cfg = {
        'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 1,
                    'train_data': {'images': '4', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
        'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'use_dropout': True},
                         'discriminator': {'filters': 4, 'n_layers': 3}},
        'checkpoint_path': str(tmp_path / 'ckpt'),
        'train_params': {'loss_type': 'tversky', 'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3,
                         'save_freq': 1, 'ema_decay': 0.999, 'metrics': True, 'save_best': 'miou', 'metric_bins': 256},
    }
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    patchgan_train(['-c', 'cfg.yaml', '-n', '2', '-b', '2', '--dataloader_workers', '0'])
    out = capsys.readouterr().out
    assert out.count('mean AP') == 4 and out.count('best threshold') == 4
    best = json.load(open(tmp_path / 'ckpt' / 'best_metrics.json'))

    def infer(gen_name, threshold, folder):
        icfg = {'dataset': {'type': 'BlobsInfer', 'dataset_path': '2', 'size': 256},
                'model_params': {'gen_filts': 4, 'disc_filts': 4, 'n_disc_layers': 3, 'activation': 'leakyrelu'},
                'checkpoint_paths': {'generator': str(tmp_path / 'ckpt' / gen_name),
                                     'discriminator': str(tmp_path / 'ckpt' / 'best_discriminator.pth')},
                'infer_params': {'output_path': str(tmp_path / folder), 'threshold': threshold}}
        (tmp_path / 'icfg.yaml').write_text(yaml.safe_dump(icfg))
        patchgan_infer(['-c', 'icfg.yaml'])
        return [np.load(tmp_path / folder / f'blob_{i:03d}.npy') for i in range(2)]

    for gen_name, entry in (('best_generator.pth', 'generator'), ('best_generator_ema.pth', 'generator_ema')):
        number = best[entry]['scores']['best_threshold'][0]
        assert 1 / 256 <= number <= 255 / 256
        a = infer(gen_name, 'best', 'pred_best_' + entry)
        b = infer(gen_name, number, 'pred_number_' + entry)
        for m, n in zip(a, b):
            assert m.shape == (256, 256) and set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(m, n)
    with pytest.raises(ValueError, match='best_generator'):
        infer('generator_ep_002.pth', 'best', 'pred_refused')
    assert not (tmp_path / 'pred_refused').exists()


# ---------------------------------------------------------------------------------------------- E. data parallel
def _dp_worker(rank, world, port, q, cout):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(4)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    t = _trainer(tempfile.mkdtemp(), cout, metrics=True, metric_bins=64)
    t.generator.eval()
    t.discriminator.eval()
    b = _batches(cout)
    x, y = torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])          # a global batch of four: two samples per rank
    xs, ys = shard_batch(x, y, rank, world)
    t.batch(xs, ys, train=False)
    m = t.read_metrics()                        # a collective: the sum over the ranks
    own = hist_ref(t._last_gen.to_nchw().cpu().numpy(), ys.numpy(), 64)
    ev = t.evaluate([(xs, ys)])
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, m['hist'], m['ignored'], own[0], own[1], ev['hist'], float(m['mean_ap'])))
    dist.destroy_process_group()


@pytest.mark.parametrize('cout', [1, 4])
def test_two_ranks_read_the_sum_of_their_histograms(cout):
    import torch.multiprocessing as mp
    from tests.test_metrics_gpu import _collect
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, cout)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, h0, i0, own0, oi0, e0, ap0), (_, h1, i1, own1, oi1, e1, ap1) = res
    assert np.array_equal(h0, h1) and i0 == i1 and (ap0 == ap1 or (np.isnan(ap0) and np.isnan(ap1)))
    assert np.array_equal(h0, own0 + own1) and i0 == oi0 + oi1
    assert h0.sum() + i0 == cout * (4 * 256 * 256 - i0) + i0
    assert np.array_equal(e0, h0) and np.array_equal(e1, h0)          # evaluate(): the same collective read
