"""Segmentation metrics on the GPU: pg_seg_confusion against the NumPy statement of its rule, exactly (A), accumulation (B),
containment (C), stream (D), the trainer's evaluation steps (E), Trainer.evaluate (F), train() with save_best (G), two data-parallel
ranks (H).  Integer counts: every comparison is np.array_equal.  Needs an MI355X."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from tests.golden_util import LOSS_KEYS
from tests.metrics_util import confusion_ref, make_case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(3, 5, 5), (2, 33, 31), (3, 256, 256)]      # 75 pixels: part of one workgroup; 2046: a ragged tail; 196608 > 512 x 256: two trips
SHAPE_IDS = ['75px', '2046px', '196608px']
_CASES = {}


def _case(N, C, H, W, soft=False):
    """One (p, y) per shape and kind, made once and shared (never modified)."""
    key = (N, C, H, W, soft)
    if key not in _CASES:
        _CASES[key] = make_case(N, C, H, W, seed=1000 + 31 * C + N * H + (7 if soft else 0), soft=soft)
    return _CASES[key]


def _counts(K, fill=None):
    t = torch.zeros(K * K + 1, dtype=torch.int64, device=DEV)
    if fill is not None:
        t += fill.to(DEV)
    return t


def _run(p, y, threshold, ld_p=None, off_p=0, ld_y=None, off_y=0, counts=None):
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view
    C = p.shape[1]
    K = 2 if C == 1 else C
    pv = to_view(torch.from_numpy(p), ld_p, off_p)
    yv = to_view(torch.from_numpy(y), ld_y, off_y)
    counts = _counts(K) if counts is None else counts
    E.seg_confusion(pv, yv, threshold, counts)
    a = counts.cpu().numpy()
    return a[:K * K].reshape(K, K), int(a[K * K])


def _check(p, y, threshold, **views):
    conf, ign = _run(p, y, threshold, **views)
    want, want_ign = confusion_ref(p, y, threshold)
    assert conf.dtype == np.int64 and np.array_equal(conf, want), (conf, want)
    assert ign == want_ign
    assert conf.sum() + ign == p.shape[0] * p.shape[2] * p.shape[3]
    return conf, ign


# ---------------------------------------------------------------------------------------------- A. exactness
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('C', [1, 2, 3, 4, 7, 32])
def test_counts_equal_numpy_dense_views(C, shape):
    N, H, W = shape
    p, y = _case(N, C, H, W)
    conf, ign = _check(p, y, 0.5)
    if 1 < C <= 7 and shape == SHAPES[2]:
        assert ign > 0 and np.count_nonzero(conf) == C * C          # the data reaches every cell and the ignore word
    if C == 1:
        _check(p, y, 0.25)
        assert not np.array_equal(confusion_ref(p, y, 0.25)[0], conf)      # (the threshold is read)


VIEWS = {
    'c4_vector_ld4': (4, dict(ld_p=4, ld_y=4)),                                  # 16-byte loads
    'c4_off3_ld7': (4, dict(ld_p=7, off_p=3, ld_y=7, off_y=3)),                  # the discriminator-input layout: by element
    'c4_off4_ld8': (4, dict(ld_p=8, off_p=4, ld_y=8, off_y=4)),                  # aligned slice of 8-float pixels
    'c4_mixed': (4, dict(ld_p=4, ld_y=7, off_y=3)),                              # one operand by vector, the other by element
    'c1_off3_ld4': (1, dict(ld_p=4, off_p=3, ld_y=4, off_y=3)),
    'c3_off2_ld6': (3, dict(ld_p=6, off_p=2, ld_y=5, off_y=1)),
}


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('name', list(VIEWS))
def test_counts_equal_numpy_channel_slices(name, shape):
    """The other channels of the wider pixels are NaN (gpu_util.to_view): a result that equals the reference did not read them."""
    C, views = VIEWS[name]
    N, H, W = shape
    p, y = _case(N, C, H, W)
    _check(p, y, 0.5, **views)
    if C == 1:
        _check(p, y, 0.25, **views)


@pytest.mark.parametrize('C', [2, 4, 7])
def test_soft_targets_take_their_argmax(C):
    N, H, W = SHAPES[1]
    p, y = _case(N, C, H, W, soft=True)
    assert ((y > 0) & (y < 1)).any()
    _check(p, y, 0.5)
    _check(p, y, 0.5, ld_p=C + 3, off_p=3, ld_y=C + 3, off_y=3)


# ---------------------------------------------------------------------------------------------- B. accumulation
@pytest.mark.parametrize('C', [1, 4])
def test_two_launches_add_to_what_the_buffer_holds(C):
    K = 2 if C == 1 else C
    p1, y1 = _case(*SHAPES[1][:1], C, *SHAPES[1][1:])
    p2, y2 = _case(*SHAPES[2][:1], C, *SHAPES[2][1:])
    # counts already there, the first next to a carry out of the low 32 bits
    before = torch.arange(K * K + 1, dtype=torch.int64) * 1000 + 5
    before[0] = (1 << 32) - 3
    counts = _counts(K, before)
    _run(p1, y1, 0.5, counts=counts)
    conf, ign = _run(p2, y2, 0.5, counts=counts)
    r1, r2 = confusion_ref(p1, y1, 0.5), confusion_ref(p2, y2, 0.5)
    b = before.numpy()
    assert np.array_equal(conf, b[:K * K].reshape(K, K) + r1[0] + r2[0])
    assert ign == b[K * K] + r1[1] + r2[1]


# ---------------------------------------------------------------------------------------------- C. containment
@pytest.mark.parametrize('name', ['c4_off3_ld7', 'c4_off4_ld8', 'c1_off3_ld4', 'c3_off2_ld6', 'c4_vector_ld4'])
def test_containment(name):
    """p and y in guarded views whose other channels are the 0xFF sentinel (NaN), counts in a guarded flat buffer: the inputs stay
    byte-identical, only the K*K + 1 words change, and the counts equal the reference (the neighbours were not read into it)."""
    from tests import guard_util as G
    from patchgan_amd import _lib as L
    C, v = VIEWS[name]
    K = 2 if C == 1 else C
    N, H, W = SHAPES[1]
    p, y = _case(N, C, H, W)
    pv, pg_ = G.view_from(torch.from_numpy(p), v.get('ld_p'), v.get('off_p', 0))
    yv, yg = G.view_from(torch.from_numpy(y), v.get('ld_y'), v.get('off_y', 0))
    cg = G.flat((K * K + 1) * 8)
    cg.inner(torch.int64).zero_()
    ins = G.Inputs()
    ins.add(pg_, 'p')
    ins.add(yg, 'y')
    torch.cuda.synchronize()
    rc = L.load().pg_seg_confusion(pv.ptr(), pv.ld, yv.ptr(), yv.ld, N, H * W, C, 0.5, cg.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    G.assert_untouched(cg, 'all', 'seg_confusion counts')
    ins.check('seg_confusion')
    a = cg.inner(torch.int64).cpu().numpy()
    want, want_ign = confusion_ref(p, y, 0.5)
    assert np.array_equal(a[:K * K].reshape(K, K), want) and a[K * K] == want_ign


# ---------------------------------------------------------------------------------------------- D. stream
def test_launch_goes_to_the_current_stream():
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view
    N, H, W = SHAPES[2]
    p, y = _case(N, 4, H, W)
    pv, yv = to_view(torch.from_numpy(p), 7, 3), to_view(torch.from_numpy(y), 7, 3)
    counts = _counts(4)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        E.seg_confusion(pv, yv, 0.5, counts)
        host = torch.empty(17, dtype=torch.int64).pin_memory()
        host.copy_(counts, non_blocking=True)
    s.synchronize()
    a = host.numpy()
    want, want_ign = confusion_ref(p, y, 0.5)
    assert np.array_equal(a[:16].reshape(4, 4), want) and a[16] == want_ign


# ---------------------------------------------------------------------------------------------- E. trainer
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
    """The segmentation loss of one step as its loss kernel wrote it (the first of the step's four device scalars)."""
    step_losses._event.synchronize()
    return float(step_losses._host[0])


@pytest.mark.parametrize('two', [False, True], ids=['one_stream', 'two_streams'])
@pytest.mark.parametrize('cout', [1, 4])
def test_evaluation_step_counts_its_own_prediction(tmp_path, cout, two):
    t = _trainer(tmp_path, cout, metrics=True, two_streams=two)
    t.generator.eval()
    t.discriminator.eval()
    x, y = _batches(cout)[0]
    t.batch(x, y, train=False)
    assert t.launch_mode == ('eager2' if two else 'eager1')
    m = t.read_metrics()
    want, want_ign = confusion_ref(t._last_gen.to_nchw().cpu().numpy(), y.numpy(), 0.5)
    assert np.array_equal(m['confusion'], want) and m['ignored'] == want_ign
    assert m['confusion'].sum() + m['ignored'] == 2 * 256 * 256
    assert (want_ign > 0) == (cout > 1)
    for k in ('iou', 'dice', 'precision', 'recall', 'pixel_acc', 'miou', 'mdice'):
        assert k in m
    assert ('iou_fg' in m) == (cout == 1)
    # a second batch adds; reset_metrics() starts over
    x2, y2 = _batches(cout)[1]
    t.batch(x2, y2, train=False)
    want2, ign2 = confusion_ref(t._last_gen.to_nchw().cpu().numpy(), y2.numpy(), 0.5)
    m2 = t.read_metrics()
    assert np.array_equal(m2['confusion'], want + want2) and m2['ignored'] == want_ign + ign2
    t.reset_metrics()
    assert t.read_metrics()['confusion'].sum() == 0
    t.metric_threshold = 0.25
    t.batch(x, y, train=False)
    want3, _ = confusion_ref(t._last_gen.to_nchw().cpu().numpy(), y.numpy(), 0.25)
    assert np.array_equal(t.read_metrics()['confusion'], want3)


@pytest.mark.parametrize('cout', [1, 4])
def test_losses_are_bit_identical_with_and_without_metrics(tmp_path, cout):
    b = _batches(cout)
    rows = {}
    for on in (None, True):
        t = _trainer(tmp_path / str(on), cout, metrics=on)
        t.setup_optimizers(1e-3, 1e-3)
        t.generator.train()
        t.discriminator.train()
        out = []
        for i, train in enumerate((True, True, False, True)):
            out.append(dict(t.batch(*b[i], train=train)))
            if on:
                if i < 2:
                    assert t.seg_counts is None                       # training steps never touch (or create) the counts
                else:
                    conf = t.read_metrics()
                    assert conf['confusion'].sum() + conf['ignored'] == 2 * 256 * 256
                    if i == 2:
                        kept = conf['confusion'].copy()
                    else:
                        assert np.array_equal(conf['confusion'], kept)
            else:
                assert t.seg_counts is None
        t.flush()
        rows[on] = out
    assert rows[None] == rows[True]
    assert all(set(r) == set(LOSS_KEYS) for r in rows[True])


# ---------------------------------------------------------------------------------------------- F. evaluate()
@pytest.mark.parametrize('cout', [1, 4])
def test_evaluate_equals_evaluation_steps(tmp_path, cout):
    t = _trainer(tmp_path, cout, metrics=True)
    g = t.generator
    g.eval()
    t.discriminator.eval()
    data = _batches(cout)[:2]
    segs = [_seg(t.batch(x, y, train=False)) for x, y in data]
    m = t.read_metrics()
    ev = t.evaluate(data)
    assert np.array_equal(ev['confusion'], m['confusion']) and ev['ignored'] == m['ignored']
    assert ev['seg_loss'] == (segs[0] + segs[1]) / 2
    assert ev['miou'] == m['miou'] or (np.isnan(ev['miou']) and np.isnan(m['miou']))
    assert np.array_equal(t.read_metrics()['confusion'], m['confusion'])          # its own counts, not the trainer's
    assert g.training is False
    g.train()
    ev2 = t.evaluate(data)
    assert g.training is True                                                      # the mode is restored
    assert np.array_equal(ev2['confusion'], ev['confusion']) and ev2['seg_loss'] == ev['seg_loss']


def test_evaluate_the_averaged_generator(tmp_path):
    import patchgan_amd as pg
    cout = 1
    t = _trainer(tmp_path, cout, ema_decay=0.9)
    t.setup_optimizers(1e-3, 1e-3)
    t.generator.train()
    t.discriminator.train()
    b = _batches(cout)
    for i in range(3):
        t.batch(*b[i], train=True)
    data = b[2:4]
    ema = t.ema_generator
    ev = t.evaluate(data, ema)
    g2 = pg.UNet(3, cout, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid')
    g2.load_state_dict(ema.state_dict())
    g2.to(DEV)
    assert g2.training
    ev2 = t.evaluate(data, g2)
    assert g2.training and not ema.training
    assert np.array_equal(ev['confusion'], ev2['confusion']) and ev['seg_loss'] == ev2['seg_loss']
    assert ev['confusion'].sum() == 2 * 2 * 256 * 256
    live = t.evaluate(data)
    assert not torch.equal(ema.flat, t.generator.flat) and live['seg_loss'] != ev['seg_loss']
    with pytest.raises(RuntimeError):
        t.evaluate(data, pg.UNet(3, 2, 4).to(DEV))


# ---------------------------------------------------------------------------------------------- G. train()
def _train_run(folder, metrics):
    t = _trainer(folder, 1, seed=21, ema_decay=0.9)
    if metrics:
        t.metrics, t.save_best = True, 'miou'
    b = _batches(1)
    ret = t.train(b[:2], b[2:4], 2, save_freq=1)
    return t, ret


def test_train_records_scores_and_keeps_the_best(tmp_path, capsys):
    import patchgan_amd as pg
    t, ret = _train_run(tmp_path / 'on', True)
    printed = capsys.readouterr().out
    assert printed.count('Validation metrics') == 2 and 'averaged generator' in printed
    folder = t.savefolder
    h = t.val_history
    assert [e['epoch'] for e in h] == [1, 2]
    for e in h:
        for k in LOSS_KEYS + ['iou', 'dice', 'precision', 'recall', 'pixel_acc', 'miou', 'mdice', 'iou_fg', 'dice_fg', 'confusion', 'ignored']:
            assert k in e, k
        assert e['confusion'].sum() == 2 * 2 * 256 * 256
        for k in ('seg_loss', 'miou', 'mdice', 'pixel_acc', 'confusion'):
            assert k in e['ema'], k
    best = json.load(open(os.path.join(folder, 'best_metrics.json')))
    assert best['metric'] == 'miou'
    k = 1 if not h[1]['miou'] > h[0]['miou'] else 2
    assert best['generator']['epoch'] == k and best['generator']['score'] == h[k - 1]['miou']
    ke = 1 if not h[1]['ema']['miou'] > h[0]['ema']['miou'] else 2
    assert best['generator_ema']['epoch'] == ke and best['generator_ema']['score'] == h[ke - 1]['ema']['miou']
    for net in ('generator', 'discriminator'):
        a = torch.load(os.path.join(folder, f'best_{net}.pth'), map_location='cpu')
        e = torch.load(os.path.join(folder, f'{net}_ep_{k:03d}.pth'), map_location='cpu')
        assert set(a) == set(e) and all(torch.equal(a[key], e[key]) for key in a), net
    g2 = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid')
    g2.load_state_dict(torch.load(os.path.join(folder, 'best_generator_ema.pth'), map_location='cpu'))
    a = torch.load(os.path.join(folder, 'best_generator_ema.pth'), map_location='cpu')
    e = torch.load(os.path.join(folder, f'generator_ema_ep_{ke:03d}.pth'), map_location='cpu')
    assert all(torch.equal(a[key], e[key]) for key in a)
    # a resumed trainer competes with the stored best
    t3 = _trainer(folder, 1, seed=21)
    t3.load_last_checkpoint()
    assert t3.start == 3 and t3._best.best['generator']['epoch'] == k

    # off: the parent's behaviour -- no file, no history, the same training
    t2, ret2 = _train_run(tmp_path / 'off', False)
    assert t2.val_history == [] and t2.seg_counts is None
    assert not [f for f in os.listdir(t2.savefolder) if f.startswith('best_')]
    assert 'Validation metrics' not in capsys.readouterr().out
    assert ret2 == ret


def test_cli_trains_with_metrics_and_infers_from_the_best_files(tmp_path, monkeypatch, capsys):
    """A YAML with metrics, save_best and ema_decay trains through patchgan_train: per-epoch scores of both generators are printed, the
    best_* files land beside the epoch checkpoints, and patchgan_infer loads best_generator*.pth as they are."""
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
                         'save_freq': 1, 'ema_decay': 0.999, 'metrics': True, 'save_best': 'miou'},
    }
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    G_ep, D_ep = patchgan_train(['-c', 'cfg.yaml', '-n', '2', '-b', '2', '--dataloader_workers', '0'])
    assert len(G_ep) == 2 and all(np.isfinite(G_ep)) and all(np.isfinite(D_ep))
    out = capsys.readouterr().out
    assert out.count('Validation metrics -- mIoU') == 2 and out.count('averaged generator: mIoU') == 2 and 'mDice' in out
    files = set(os.listdir(tmp_path / 'ckpt'))
    assert {'best_generator.pth', 'best_generator_ema.pth', 'best_discriminator.pth', 'best_metrics.json'} <= files
    assert {f'{net}_ep_{ep:03d}.pth' for net in ('discriminator', 'generator_ema', 'generator') for ep in (1, 2)} <= files
    for name in ('best_generator.pth', 'best_generator_ema.pth'):
        icfg = {'dataset': {'type': 'BlobsInfer', 'dataset_path': '2', 'size': 256},
                'model_params': {'gen_filts': 4, 'disc_filts': 4, 'n_disc_layers': 3, 'activation': 'leakyrelu'},
                'checkpoint_paths': {'generator': str(tmp_path / 'ckpt' / name),
                                     'discriminator': str(tmp_path / 'ckpt' / 'best_discriminator.pth')},
                'infer_params': {'output_path': str(tmp_path / ('pred_' + name)), 'threshold': 0.5}}
        (tmp_path / 'icfg.yaml').write_text(yaml.safe_dump(icfg))
        patchgan_infer(['-c', 'icfg.yaml'])
        for i in range(2):
            m = np.load(tmp_path / ('pred_' + name) / f'blob_{i:03d}.npy')
            assert m.shape == (256, 256) and set(np.unique(m)) <= {0.0, 1.0}


# ---------------------------------------------------------------------------------------------- H. data parallel
def _dp_worker(rank, world, port, q, cout):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(4)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    t = _trainer(tempfile.mkdtemp(), cout, metrics=True)
    t.generator.eval()
    t.discriminator.eval()
    b = _batches(cout)
    x, y = torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])          # a global batch of four: two samples per rank
    xs, ys = shard_batch(x, y, rank, world)
    t.batch(xs, ys, train=False)
    m = t.read_metrics()                        # a collective: the sum over the ranks
    own = confusion_ref(t._last_gen.to_nchw().cpu().numpy(), ys.numpy(), 0.5)
    ev = t.evaluate([(xs, ys)])
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, m['confusion'], m['ignored'], own[0], own[1], ev['confusion'], ev['ignored']))
    dist.destroy_process_group()


def _collect(q, procs, timeout=300.0):
    """One result per worker; fails at once when a worker died, and leaves no rank behind on the GPU."""
    import queue
    import time
    out, t0 = [], time.monotonic()
    try:
        while len(out) < len(procs):
            try:
                out.append(q.get(timeout=1.0))
                continue
            except queue.Empty:
                pass
            dead = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
            assert not dead, f'worker(s) died (rank, exit code): {dead}'
            assert time.monotonic() - t0 < timeout, 'workers still running after the timeout'
    except BaseException:
        for p in procs:
            if p.is_alive():
                p.kill()
        raise
    return sorted(out, key=lambda r: r[0])


@pytest.mark.parametrize('cout', [1, 4])
def test_two_ranks_read_the_sum_of_their_counts(cout):
    """Each rank runs one evaluation step on its shard; read_metrics() gives both the same matrix, the sum of what each counted on
    its own prediction.  (No comparison against a one-process run: batch N and batch 2N may take different convolution kernels, and
    one ulp flips a pixel at the threshold.)"""
    import torch.multiprocessing as mp
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
    (_, c0, i0, own0, oi0, e0, ei0), (_, c1, i1, own1, oi1, e1, ei1) = res
    assert np.array_equal(c0, c1) and i0 == i1
    assert np.array_equal(c0, own0 + own1) and i0 == oi0 + oi1
    assert c0.sum() + i0 == 4 * 256 * 256 and own0.sum() + oi0 == 2 * 256 * 256
    assert np.array_equal(e0, c0) and np.array_equal(e1, c0) and ei0 == ei1 == i0          # evaluate(): the same collective read
