"""Score curves without a GPU: the NumPy statement of the histogram rule on hand-worked inputs, metrics.curve against thresholding the
predictions directly, average precision and the best threshold by hand, the C ABI's argument validation (before any launch), the
trainer's settings, SegHist.read under a gloo world of 2, and what best_metrics.json carries into patchgan_infer."""
import json
import os
import re
import socket
import warnings

import numpy as np
import pytest
import torch
import yaml

from tests.metrics_util import confusion_ref
from tests.seghist_util import curve_ref, edge_case, edge_values, hist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(values):
    """values -> [1, 1, 1, n] float32"""
    return np.asarray(values, dtype=np.float32).reshape(1, 1, 1, -1)


# ---------------------------------------------------------------------------------------------- 1. the histogram rule, by hand
def test_ref_value_on_a_threshold_lands_in_the_upper_bin_and_the_clamps_hold():
    f = np.float32
    below = np.nextafter(f(0.25), f(0))
    p = _row([0.25, below, 1.0, 1.5, -0.25, -0.0, 1e-45, np.nextafter(f(1), f(0)), 0.0])
    y = _row([1, 1, 0, 1, 0, 1, 0, 1, 0.5])           # (a target of exactly 0.5 is foreground)
    hist, ign = hist_ref(p, y, 16)
    want = np.zeros((1, 2, 16), dtype=np.int64)
    for t, b in ((1, 4), (1, 3), (0, 15), (1, 15), (0, 0), (1, 0), (0, 0), (1, 15), (1, 0)):
        want[0, t, b] += 1
    assert ign == 0 and hist.dtype == np.int64 and np.array_equal(hist, want)


def test_ref_tie_in_the_target_goes_to_the_lower_index_and_a_zero_pixel_is_ignored():
    # four pixels, three channels; bins of 16: 0.5 -> 8, 0.125 -> 2, 0.9 -> 14
    p = np.asarray([[[0.5, 0.125, 0.9, 0.5]], [[0.125, 0.5, 0.5, 0.9]], [[0.9, 0.9, 0.125, 0.125]]], dtype=np.float32)[None]
    y = np.asarray([[[0.5, 0.0, 0.0, 0.0]], [[0.5, 0.25, 0.0, -1.0]], [[0.0, 0.25, 0.0, 0.0]]], dtype=np.float32)[None]
    # labels: pixel 0 -> class 0 (tie 0/1), pixel 1 -> class 1 (tie 1/2), pixel 2 all zero: ignored, pixel 3 largest 0: ignored
    hist, ign = hist_ref(p, y, 16)
    want = np.zeros((3, 2, 16), dtype=np.int64)
    for c, t, b in ((0, 1, 8), (1, 0, 2), (2, 0, 14), (0, 0, 2), (1, 1, 8), (2, 0, 14)):
        want[c, t, b] += 1
    assert ign == 2 and np.array_equal(hist, want)
    assert hist.sum() + ign == 3 * 2 + 2


def test_edge_recipe_holds_what_it_promises():
    v = edge_values(16)
    f = np.float32
    assert v.dtype == np.float32
    for k in range(17):
        x = f(k / 16)
        assert x in v and np.nextafter(x, f(2)) in v and np.nextafter(x, f(-2)) in v
    assert f(1e-45) in v and f(1e-45) > 0 and (v > 1).any() and (v < 0).any() and np.nextafter(f(1), f(0)) in v
    assert np.signbit(v[v == 0]).any()


# ---------------------------------------------------------------------------------------------- 2. curve()
@pytest.mark.parametrize('bins', [16, 256])
@pytest.mark.parametrize('C', [1, 3])
def test_curve_of_the_histogram_equals_thresholding_the_predictions(C, bins):
    from patchgan_amd.metrics import curve
    p, y = edge_case(C, bins, seed=5 + C + bins)
    hist, ign = hist_ref(p, y, bins)
    assert hist.sum() + ign == C * (p[0, 0].size - ign) + ign
    cv = curve(hist)['curve']
    want = curve_ref(p, y, bins)
    for k in ('tp', 'fp', 'fn', 'tn'):
        assert cv[k].dtype == np.int64 and np.array_equal(cv[k], want[k]), k
    assert np.array_equal(cv['thresholds'], np.arange(bins) / bins)


@pytest.mark.parametrize('bins', [16, 256, 1024])
def test_one_channel_counts_equal_the_confusion_matrix_at_every_threshold(bins):
    from patchgan_amd.metrics import curve
    p, y = edge_case(1, bins, seed=9 + bins, repeat=1)
    cv = curve(hist_ref(p, y, bins)[0])['curve']
    for k in range(1, bins):
        conf, _ = confusion_ref(p, y, k / bins)
        got = [[cv['tn'][0, k], cv['fp'][0, k]], [cv['fn'][0, k], cv['tp'][0, k]]]
        assert np.array_equal(conf, got), k


def test_average_precision_of_six_pixels_by_hand():
    from patchgan_amd.metrics import curve
    # bins of 16:   14     12    11    9     4    1
    p = _row([0.9, 0.8, 0.7, 0.6, 0.3, 0.1])
    y = _row([1, 0, 1, 1, 0, 1])
    out = curve(hist_ref(p, y, 16)[0])
    cv = out['curve']
    # recall steps of 1/4 at k = 14, 11, 9, 1 with precision 1/1, 2/3, 3/4, 4/6; k = 15 predicts nothing: no precision, no step
    assert np.isnan(cv['precision'][0, 15]) and cv['recall'][0, 15] == 0
    assert abs(out['ap'][0] - (1 + 2 / 3 + 3 / 4 + 4 / 6) / 4) < 1e-15 and abs(out['mean_ap'] - 37 / 48) < 1e-15
    assert np.array_equal(cv['tp'][0], [4, 4] + [3] * 8 + [2] * 2 + [1] * 3 + [0])
    assert np.array_equal(cv['fp'][0], [2, 2, 2, 2, 2] + [1] * 8 + [0] * 3)
    assert np.array_equal(cv['fn'][0], 4 - cv['tp'][0]) and np.array_equal(cv['tn'][0], 2 - cv['fp'][0])
    assert abs(cv['iou'][0, 9] - 3 / 5) < 1e-15 and abs(cv['dice'][0, 9] - 6 / 8) < 1e-15
    # the best IoU is 4/6 at k = 1 (and at k = 0, which does not count)
    assert out['best_threshold'][0] == 1 / 16 and abs(out['best_iou'][0] - 4 / 6) < 1e-15 and abs(out['best_dice'][0] - 8 / 10) < 1e-15
    assert out['best_miou'] == out['best_iou'][0]
    for k in ('precision', 'recall', 'iou', 'dice'):
        assert cv[k].dtype == np.float64 and cv[k].shape == (1, 16)


def test_best_threshold_takes_the_smallest_k_of_a_tie_and_never_k_0():
    from patchgan_amd.metrics import curve
    # bins of 16: 0.6 -> 9 (positive), 0.3 -> 4 (negative): IoU 1/2 for k <= 4, 1 for k = 5 .. 9, 0 above
    out = curve(hist_ref(_row([0.6, 0.3]), _row([1, 0]), 16)[0])
    assert out['best_threshold'][0] == 5 / 16 and out['best_iou'][0] == 1.0
    # one positive pixel: IoU 1 for k = 0 .. 9 -- k = 0 is left out
    out = curve(hist_ref(_row([0.6]), _row([1]), 16)[0])
    assert out['curve']['iou'][0, 0] == 1.0 and out['best_threshold'][0] == 1 / 16


def test_absent_class_and_empty_table_are_nan_without_a_warning():
    from patchgan_amd.metrics import curve
    h = np.zeros((2, 2, 16), dtype=np.int64)
    h[0, 1, 12] = 3
    h[0, 0, 2] = 5
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        out = curve(h)
        empty = curve(np.zeros((3, 2, 16), dtype=np.int64))
    assert np.isnan(out['curve']['iou'][1]).all() and np.isnan(out['best_threshold'][1]) and np.isnan(out['ap'][1])
    assert np.isnan(out['best_iou'][1]) and np.isnan(out['best_dice'][1])
    assert out['ap'][0] == 1.0 and out['mean_ap'] == 1.0 and out['best_threshold'][0] == 3 / 16 and out['best_miou'] == 1.0
    for k in ('ap', 'best_threshold', 'best_iou', 'best_dice'):
        assert np.isnan(empty[k]).all(), k
    assert np.isnan(empty['mean_ap']) and np.isnan(empty['best_miou'])
    for k in ('precision', 'recall', 'iou', 'dice'):
        assert np.isnan(empty['curve'][k]).all(), k
    # a class with negatives only: IoU 0 where it is predicted, no recall, no AP
    h = np.zeros((1, 2, 16), dtype=np.int64)
    h[0, 0, 7] = 2
    out = curve(h)
    assert out['curve']['iou'][0, 7] == 0.0 and np.isnan(out['curve']['iou'][0, 8]) and np.isnan(out['ap'][0])
    with pytest.raises(ValueError):
        curve(np.zeros((2, 16)))


# ---------------------------------------------------------------------------------------------- 3. C ABI
def test_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in ('pg_seg_hist', 'pg_seg_hist_max_words'):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.pg_seg_hist_max_words() == 8192


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host
    EINVAL = -1

    def call(p=a, ld_p=4, y=a, ld_y=4, N=2, HW=64, C=4, bins=16, hist=a):
        return lib.pg_seg_hist(p, ld_p, y, ld_y, N, HW, C, bins, hist, None)
    assert call(p=None) == EINVAL and call(y=None) == EINVAL and call(hist=None) == EINVAL
    for bad in (0, -1):
        assert call(N=bad) == EINVAL and call(HW=bad) == EINVAL and call(C=bad) == EINVAL and call(bins=bad) == EINVAL
    assert call(C=33, ld_p=33, ld_y=33) == EINVAL
    for bins in (1, 8, 15, 17, 24, 48, 100, 255, 1000, 1023, 1025, 2048, 1 << 30):
        assert call(bins=bins) == EINVAL, bins
    assert call(C=32, ld_p=32, ld_y=32, bins=512) == EINVAL          # 16384 > pg_seg_hist_max_words()
    assert call(C=9, ld_p=9, ld_y=9, bins=1024) == EINVAL
    assert call(ld_p=3) == EINVAL and call(ld_y=3) == EINVAL
    assert call(C=1, ld_p=0, ld_y=1) == EINVAL and call(C=1, ld_p=1, ld_y=0) == EINVAL


# ---------------------------------------------------------------------------------------------- 4. settings
def _trainer(folder):
    import patchgan_amd as pg
    torch.manual_seed(3)
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    return pg.Trainer(g, d, str(folder))


def test_defaults_are_off(tmp_path):
    import patchgan_amd as pg
    assert pg.Trainer.metric_bins is None
    t = _trainer(tmp_path)
    assert t.metric_bins is None and t.seg_hist is None
    import patchgan.metrics as alias
    import patchgan_amd.metrics as M
    assert alias.curve is M.curve and alias.SegHist is M.SegHist and alias.best_threshold is M.best_threshold


TRAIN_YAML = """
train_params:
  loss_type: tversky
  seg_alpha: 200
  gen_learning_rate: 1.e-3
  disc_learning_rate: 1.e-3
  metrics: true
  metric_bins: 256
"""


def test_yaml_key_reaches_the_trainer(tmp_path):
    from patchgan_amd.train import apply_train_params
    cfg = yaml.safe_load(TRAIN_YAML)['train_params']
    t = _trainer(tmp_path)
    apply_train_params(t, cfg)
    assert t.metrics is True and t.metric_bins == 256
    del cfg['metric_bins']          # absent = off
    apply_train_params(t, cfg)
    assert t.metric_bins is None


def test_metric_bins_needs_metrics_and_a_power_of_two(tmp_path):
    t = _trainer(tmp_path)
    t.metric_bins = 256
    with pytest.raises(ValueError, match='needs Trainer.metrics = True'):
        t.train([], [], 1)
    t.metrics = True
    for bad in (100, 8, 2048, 0, 'many', 64.0, True):
        t.metric_bins = bad
        with pytest.raises(ValueError, match='metric_bins'):
            t.train([], [], 1)
    for good in (16, 256, 1024):
        t.metric_bins = good
        assert t._metric_bins() == good


# ---------------------------------------------------------------------------------------------- 5. SegHist
def _hist_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    from patchgan_amd.metrics import SegHist
    from patchgan_amd.parallel import current
    h = SegHist(3, 16, 'cpu')
    h.t += torch.arange(97, dtype=torch.int64) * (rank + 1)
    hist, ign = h.read(current())
    again, _ = h.read()                        # (the default finds the group itself; the rank's own counts were not overwritten)
    q.put((rank, hist, ign, again, h.t.clone().numpy()))
    dist.destroy_process_group()


def test_seghist_read_sums_over_the_ranks():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_hist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.arange(97, dtype=np.int64) * 3
    for rank, hist, ign, again, own in res:
        assert hist.dtype == np.int64 and hist.shape == (3, 2, 16)
        assert np.array_equal(hist, want[:96].reshape(3, 2, 16)) and ign == 288 and np.array_equal(again, hist)
        assert np.array_equal(own, np.arange(97) * (rank + 1))


def test_seghist_without_a_group():
    from patchgan_amd.metrics import SegHist
    h = SegHist(1, 16, 'cpu')
    assert (h.C, h.bins) == (1, 16) and h.t.dtype == torch.int64 and h.t.numel() == 33
    h.t += torch.arange(33)
    hist, ign = h.read()
    assert np.array_equal(hist, np.arange(32).reshape(1, 2, 16)) and ign == 32
    assert int(h.zero_().t.sum()) == 0
    for C, bins in ((33, 16), (0, 16), (1, 100), (1, 8), (1, 2048), (32, 512)):
        with pytest.raises(ValueError):
            SegHist(C, bins, 'cpu')
    assert SegHist(32, 256, 'cpu').t.numel() == 32 * 2 * 256 + 1


# ---------------------------------------------------------------------------------------------- 6. best_metrics.json
def _report(p, y, bins=16, threshold=0.5):
    from patchgan_amd.metrics import report, report_curve
    return dict(report(*confusion_ref(p, y, threshold)), **report_curve(hist_ref(p, y, bins)[0]))


def test_tracker_stores_the_best_threshold_without_the_arrays(tmp_path):
    from patchgan_amd.metrics import BestTracker
    rep = _report(_row([0.9, 0.8, 0.7, 0.6, 0.3, 0.1]), _row([1, 0, 1, 1, 0, 1]))
    assert 'curve' in rep and rep['hist'].shape == (1, 2, 16)
    b = BestTracker('miou')
    assert b.update('generator', 4, rep)
    d = json.load(open(b.save(str(tmp_path))))
    s = d['generator']['scores']
    assert s['best_threshold'] == [1 / 16] and s['best_iou'] == [4 / 6] and abs(s['mean_ap'] - 37 / 48) < 1e-15 and s['ap'] == [s['mean_ap']]
    assert 'curve' not in s and 'hist' not in s and 'confusion' in s
    text = open(os.path.join(str(tmp_path), 'best_metrics.json')).read()
    assert 'thresholds' not in text and 'precision' in s and len(s['precision']) == 2          # (scores() of the matrix: per class)
    b2 = BestTracker.load(str(tmp_path))
    assert b2.best == b.best


def _best_file(folder, **entries):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'best_metrics.json'), 'w') as f:
        json.dump(dict({'metric': 'miou'}, **entries), f)


def _entry(**scores):
    return {'epoch': 2, 'score': 0.5, 'scores': dict({'miou': 0.5}, **scores)}


def test_best_threshold_lookup_accepts_and_refuses(tmp_path):
    from patchgan_amd.metrics import best_threshold
    a = str(tmp_path / 'a')
    _best_file(a, generator=_entry(best_threshold=[0.3125]), generator_ema=_entry(best_threshold=[0.4375]))
    assert best_threshold(os.path.join(a, 'best_generator.pth'), 1) == 0.3125
    assert best_threshold(os.path.join(a, 'best_generator_ema.pth'), 1) == 0.4375
    # another epoch's weights, whatever the file beside them says
    for name in ('generator_ep_002.pth', 'generator_ema_ep_002.pth', 'best_discriminator.pth', 'generator.pth'):
        with pytest.raises(ValueError, match='best_generator'):
            best_threshold(os.path.join(a, name), 1)
    # several output channels
    with pytest.raises(ValueError, match='one output channel'):
        best_threshold(os.path.join(a, 'best_generator.pth'), 4)
    # no file
    with pytest.raises(ValueError, match='best_metrics.json'):
        best_threshold(str(tmp_path / 'none' / 'best_generator.pth'), 1)
    # no entry for that model
    b = str(tmp_path / 'b')
    _best_file(b, generator=_entry(best_threshold=[0.25]))
    assert best_threshold(os.path.join(b, 'best_generator.pth'), 1) == 0.25
    with pytest.raises(ValueError, match='generator_ema'):
        best_threshold(os.path.join(b, 'best_generator_ema.pth'), 1)
    # an entry written without metric_bins, and one whose threshold is null (no IoU at any threshold)
    c = str(tmp_path / 'c')
    _best_file(c, generator=_entry(), generator_ema=_entry(best_threshold=[None]))
    for name in ('best_generator.pth', 'best_generator_ema.pth'):
        with pytest.raises(ValueError, match='best_threshold'):
            best_threshold(os.path.join(c, name), 1)
