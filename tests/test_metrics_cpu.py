"""Segmentation metrics without a GPU: the NumPy statement of the counting rule on hand-worked inputs, scores() against hand-computed
values, the C ABI's argument validation (before any launch), the trainer's plumbing and best-so-far rule, and SegCounts.read under a
gloo world of 2."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


def _nchw(channels):
    """channels: list of 2 x 3 arrays -> [1, C, 2, 3] float32"""
    return np.asarray(channels, dtype=np.float32)[None]


# ---------------------------------------------------------------------------------------------- 1. the counting rule, by hand
def test_ref_tie_between_channels_takes_the_lower_index():
    p = _nchw([[[0.5, 0.2, 0.1], [0.3, 0.3, 0.0]],
               [[0.5, 0.7, 0.1], [0.3, 0.1, 0.0]],
               [[0.1, 0.7, 0.1], [0.3, 0.3, 0.0]]])
    # argmax per pixel, first maximum:  0 1 0 / 0 0 0   (ties at five of the six pixels)
    y = _nchw([[[0, 0, 1], [0, 1, 0]],
               [[1, 0, 0], [0, 0, 1]],
               [[0, 1, 0], [1, 0, 0]]])
    # true class:                       1 2 0 / 2 0 1
    conf, ign = confusion_ref(p, y, 0.5)
    want = np.zeros((3, 3), dtype=np.int64)
    for t, q in ((1, 0), (2, 1), (0, 0), (2, 0), (0, 0), (1, 0)):
        want[t, q] += 1
    assert ign == 0 and conf.dtype == np.int64 and np.array_equal(conf, want)


def test_ref_prediction_equal_to_the_threshold_is_foreground():
    p = _nchw([[[0.5, 0.49999997, 0.25], [0.75, 0.0, 0.5]]])
    y = _nchw([[[1, 1, 0], [0, 0.5, 0.49]]])          # (a target of exactly 0.5 is foreground too)
    conf, ign = confusion_ref(p, y, 0.5)
    # (t, q): (1,1) (1,0) (0,0) / (0,1) (1,0) (0,1)
    assert ign == 0 and np.array_equal(conf, [[1, 2], [2, 1]])
    conf, _ = confusion_ref(p, y, 0.25)               # 0.25 >= 0.25
    assert np.array_equal(conf, [[0, 3], [1, 2]])


def test_ref_all_zero_target_pixel_is_ignored():
    p = _nchw([[[0.9, 0.1, 0.2], [0.3, 0.6, 0.5]],
               [[0.1, 0.9, 0.8], [0.7, 0.4, 0.5]]])
    # predicted:                        0 1 1 / 1 0 0
    y = _nchw([[[1, 0, 0], [0, 0, 0]],
               [[0, 0, 1], [1, 0, -1]]])
    # true:                             0 - 1 / 1 - -   (the last pixel's largest target is 0: ignored as well)
    conf, ign = confusion_ref(p, y, 0.5)
    assert ign == 3 and np.array_equal(conf, [[1, 0], [0, 2]]) and conf.sum() + ign == 6


def test_ref_soft_target_takes_its_argmax():
    p = _nchw([[[0.2, 0.2, 0.9], [0.1, 0.5, 0.3]],
               [[0.7, 0.1, 0.0], [0.8, 0.4, 0.3]]])
    # predicted:                        1 0 0 / 1 0 0
    y = _nchw([[[0.3, 0.6, 0.5], [0.125, 0.0, 0.25]],
               [[0.6, 0.4, 0.5], [0.875, 0.0, 0.125]]])
    # true:                             1 0 0 / 1 - 0
    conf, ign = confusion_ref(p, y, 0.5)
    assert ign == 1 and np.array_equal(conf, [[3, 0], [0, 2]])


# ---------------------------------------------------------------------------------------------- 2. scores
def test_scores_2x2_by_hand():
    from patchgan_amd.metrics import scores
    s = scores(np.array([[50, 10], [5, 35]]))          # class 1: tp 35, fp 10, fn 5; class 0: tp 50, fp 5, fn 10
    assert np.allclose(s['iou'], [50 / 65, 35 / 50], rtol=0, atol=1e-15)
    assert np.allclose(s['dice'], [100 / 115, 70 / 85], rtol=0, atol=1e-15)
    assert np.allclose(s['precision'], [50 / 55, 35 / 45], rtol=0, atol=1e-15)
    assert np.allclose(s['recall'], [50 / 60, 35 / 40], rtol=0, atol=1e-15)
    assert s['pixel_acc'] == 85 / 100
    assert abs(s['miou'] - (50 / 65 + 35 / 50) / 2) < 1e-15 and abs(s['mdice'] - (100 / 115 + 70 / 85) / 2) < 1e-15
    assert s['iou_fg'] == s['iou'][1] and s['dice_fg'] == s['dice'][1]
    assert s['iou'].dtype == np.float64


def test_scores_3x3_with_an_absent_class():
    from patchgan_amd.metrics import scores
    # class 2 appears neither in the target (row) nor in the prediction (column)
    s = scores(np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]]))
    assert np.allclose(s['iou'][:2], [6 / 9, 3 / 6], rtol=0, atol=1e-15) and np.isnan(s['iou'][2])
    assert np.isnan(s['dice'][2]) and np.isnan(s['precision'][2]) and np.isnan(s['recall'][2])
    assert abs(s['miou'] - (6 / 9 + 3 / 6) / 2) < 1e-15          # the absent class is left out of the mean
    assert abs(s['mdice'] - (12 / 15 + 6 / 9) / 2) < 1e-15
    assert s['pixel_acc'] == 9 / 12
    assert 'iou_fg' not in s
    # a class that is predicted but never true: precision 0 / n, recall nan, IoU 0 (it counts in the mean)
    s = scores(np.array([[4, 0, 1], [0, 5, 2], [0, 0, 0]]))
    assert s['iou'][2] == 0.0 and s['precision'][2] == 0.0 and np.isnan(s['recall'][2])
    assert abs(s['miou'] - (4 / 5 + 5 / 7 + 0) / 3) < 1e-15


def test_scores_of_an_empty_matrix_are_nan_without_a_warning():
    from patchgan_amd.metrics import scores
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        s = scores(np.zeros((3, 3), dtype=np.int64))
    for k in ('iou', 'dice', 'precision', 'recall'):
        assert np.isnan(s[k]).all(), k
    assert np.isnan(s['pixel_acc']) and np.isnan(s['miou']) and np.isnan(s['mdice'])


def test_dice_is_2iou_over_1_plus_iou():
    from patchgan_amd.metrics import scores
    rng = np.random.default_rng(5)
    for i in range(100):
        K = int(rng.integers(2, 8))
        c = rng.integers(0, 1000, size=(K, K))
        if i % 10 == 0:
            c[:, 0] = 0
            c[0, :] = 0          # an absent class: nan on both sides
        s = scores(c)
        want = 2 * s['iou'] / (1 + s['iou'])
        assert np.array_equal(np.isnan(want), np.isnan(s['dice']))
        ok = ~np.isnan(want)
        assert np.abs(s['dice'][ok] - want[ok]).max() <= 4 * np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------- 3. C ABI
def test_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in ('pg_seg_confusion', 'pg_seg_confusion_max_c'):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.pg_seg_confusion_max_c() == 32


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host
    EINVAL = -1

    def call(p=a, ld_p=4, y=a, ld_y=4, N=2, HW=64, C=4, counts=a):
        return lib.pg_seg_confusion(p, ld_p, y, ld_y, N, HW, C, 0.5, counts, None)
    assert call(p=None) == EINVAL and call(y=None) == EINVAL and call(counts=None) == EINVAL
    for bad in (0, -1):
        assert call(N=bad) == EINVAL and call(HW=bad) == EINVAL and call(C=bad) == EINVAL
    assert call(C=33, ld_p=33, ld_y=33) == EINVAL
    assert call(ld_p=3) == EINVAL and call(ld_y=3) == EINVAL
    assert call(C=1, ld_p=0, ld_y=1) == EINVAL and call(C=1, ld_p=1, ld_y=0) == EINVAL


# ---------------------------------------------------------------------------------------------- 4. trainer plumbing
def _trainer(folder):
    import patchgan_amd as pg
    torch.manual_seed(3)
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    return pg.Trainer(g, d, str(folder))


def test_defaults_are_off(tmp_path):
    import patchgan_amd as pg
    assert pg.Trainer.metrics is None and pg.Trainer.save_best is None and pg.Trainer.metric_threshold == 0.5
    t = _trainer(tmp_path)
    assert t.metrics is None and t.save_best is None and t.seg_counts is None and t.val_history == []
    import patchgan.metrics as alias
    import patchgan_amd.metrics as M
    assert alias.scores is M.scores and alias.SegCounts is M.SegCounts


TRAIN_YAML = """
train_params:
  loss_type: tversky
  seg_alpha: 200
  gen_learning_rate: 1.e-3
  disc_learning_rate: 1.e-3
  metrics: true
  metric_threshold: 0.25
  save_best: mdice
"""


def test_yaml_keys_reach_the_trainer(tmp_path):
    from patchgan_amd.train import apply_train_params
    cfg = yaml.safe_load(TRAIN_YAML)['train_params']
    t = _trainer(tmp_path)
    apply_train_params(t, cfg)
    assert t.metrics is True and t.metric_threshold == 0.25 and t.save_best == 'mdice'
    for k in ('metrics', 'metric_threshold', 'save_best'):          # absent = off
        del cfg[k]
    apply_train_params(t, cfg)
    assert t.metrics is None and t.metric_threshold == 0.5 and t.save_best is None


def test_save_best_needs_metrics(tmp_path):
    t = _trainer(tmp_path)
    t.save_best = 'miou'
    with pytest.raises(ValueError, match='metrics'):
        t.train([], [], 1)
    t.metrics = True
    t.save_best = 'accuracy'
    with pytest.raises(ValueError, match='save_best'):
        t.train([], [], 1)


def test_best_so_far_rule(tmp_path):
    from patchgan_amd.metrics import BestTracker, scores
    b = BestTracker('miou')
    s = lambda v: {'miou': v, 'mdice': 0.5, 'iou': np.array([v, NAN])}
    assert not b.update('generator', 1, s(NAN))                    # nan never wins, not even against nothing
    assert 'generator' not in b.best
    assert b.update('generator', 2, s(0.4))
    assert not b.update('generator', 3, s(0.4))                    # strictly greater only
    assert not b.update('generator', 4, s(NAN)) and not b.update('generator', 5, s(0.3))
    assert b.update('generator', 6, s(0.41)) and b.best['generator']['epoch'] == 6
    assert b.update('generator_ema', 3, s(0.2)) and b.best['generator']['score'] == 0.41      # tracked independently
    # JSON round trip: a plain dict, nan stored as null
    path = b.save(str(tmp_path))
    assert os.path.basename(path) == 'best_metrics.json'
    d = json.load(open(path))
    assert d['metric'] == 'miou' and d['generator'] == {'epoch': 6, 'score': 0.41, 'scores': {'miou': 0.41, 'mdice': 0.5, 'iou': [0.41, None]}}
    b2 = BestTracker.load(str(tmp_path))
    assert b2.metric == 'miou' and b2.best == b.best
    assert not b2.update('generator', 7, s(0.40)) and b2.update('generator', 8, s(0.5))
    assert BestTracker.load(str(tmp_path / 'nowhere')) is None
    # a full score dict serialises
    b.update('generator', 9, dict(scores(np.array([[3, 1], [0, 0]])), confusion=np.array([[3, 1], [0, 0]]), ignored=0))
    json.load(open(b.save(str(tmp_path))))


def test_resume_keeps_a_better_stored_score(tmp_path):
    """load_last_checkpoint() reads best_metrics.json back: the resumed run's first, worse epoch does not replace the stored best."""
    from patchgan_amd.metrics import BestTracker
    t = _trainer(tmp_path)
    t.save(3)
    b = BestTracker('miou')
    b.update('generator', 2, {'miou': 0.8, 'mdice': 0.9})
    b.save(t.savefolder)
    t2 = _trainer(tmp_path)
    assert t2._best is None
    t2.load_last_checkpoint()
    assert t2.start == 4 and t2._best.metric == 'miou' and t2._best.best['generator']['score'] == 0.8
    assert not t2._best.update('generator', 4, {'miou': 0.7, 'mdice': 0.95})
    # none of the new files is taken for an epoch checkpoint
    for name in ('best_generator.pth', 'best_discriminator.pth', 'best_generator_ema.pth'):
        torch.save({}, os.path.join(t.savefolder, name))
    t3 = _trainer(tmp_path)
    t3.load_last_checkpoint()
    assert t3.start == 4


# ---------------------------------------------------------------------------------------------- 5. SegCounts under a process group
def _counts_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    from patchgan_amd.metrics import SegCounts
    from patchgan_amd.parallel import current
    c = SegCounts(3, 'cpu')
    c.t += torch.arange(10, dtype=torch.int64) * (rank + 1)
    conf, ign = c.read(current())
    again, _ = c.read()                        # (the default finds the group itself; the rank's own counts were not overwritten)
    q.put((rank, conf, ign, again, c.t.clone().numpy()))
    dist.destroy_process_group()


def test_segcounts_read_sums_over_the_ranks():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_counts_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.arange(10, dtype=np.int64) * 3
    for rank, conf, ign, again, own in res:
        assert conf.dtype == np.int64 and conf.shape == (3, 3)
        assert np.array_equal(conf, want[:9].reshape(3, 3)) and ign == 27 and np.array_equal(again, conf)
        assert np.array_equal(own, np.arange(10) * (rank + 1))


def test_segcounts_without_a_group():
    from patchgan_amd.metrics import SegCounts
    c = SegCounts(1, 'cpu')
    assert c.K == 2 and c.t.dtype == torch.int64 and c.t.numel() == 5
    c.t += torch.tensor([1, 2, 3, 4, 0])
    conf, ign = c.read()
    assert np.array_equal(conf, [[1, 2], [3, 4]]) and ign == 0
    assert int(c.zero_().t.sum()) == 0
    with pytest.raises(ValueError):
        SegCounts(33, 'cpu')
