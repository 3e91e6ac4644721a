"""Gradient accumulation on the device: pg_grad_accum against its float32 NumPy replay bit for bit (tests/accum_util.py) in guarded
buffers, PG_EINVAL with live buffers, and Trainer.accumulate through whole windows: the k = 2 identity with a plain step, a k = 3 window
replayed from its own gradients, the window as the large batch, every launch mode, every optimizer option at once, the NaN skip, short
windows and discards, the untouched default trainer, and two data-parallel ranks.  Needs an MI355X."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import accum_util as A
from tests import guard_util as GU
from tests import optim_util as U
from tests.golden_util import LOSS_KEYS, Golden
from tests.gradclip_util import scaled
from tests.lossopt_util import ADAM_BIG_N

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, INF = float('nan'), float('inf')
GOLD = 'a_lrelu_tversky'
LRS = (1e-3, 2e-3)


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _nets(seed=99, spectral=False, nf=None):
    import patchgan_amd as pg
    c = Golden(GOLD).cfg
    torch.manual_seed(seed)
    g = pg.UNet(c['in_nc'], c['out_nc'], nf or c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], nf or c['ndf'], n_layers=c['n_layers'], norm=c['norm'], spectral_norm=spectral)
    g.cuda(), d.cuda()
    g.train(), d.train()
    return g, d


def _batches(steps, seed=5, B=None):
    c = Golden(GOLD).cfg
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        x = torch.rand(B or c['B'], c['in_nc'], c['size'], c['size'], generator=gen)
        out.append((x, (torch.rand(B or c['B'], c['out_nc'], c['size'], c['size'], generator=gen) > 0.7).float()))
    return out


def _trainer(folder, accumulate=None, **kw):
    """A trainer on freshly seeded networks (the same initial weights for the same seed) with its optimizers set up."""
    import patchgan_amd as pg
    attrs = {k: kw.pop(k) for k in list(kw) if k not in ('seed', 'spectral', 'nf')}
    g, d = _nets(**kw)
    t = pg.Trainer(g, d, str(folder))
    t.accumulate = accumulate
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers(*LRS)
    return t


def _settle(t):
    t.flush()
    torch.cuda.synchronize()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _state(t):
    """(G.flat, D.flat, the four moments [, the weight average]) as NumPy copies, everything in flight completed."""
    _settle(t)
    bufs = (t.generator.flat, t.discriminator.flat) + tuple(t._adam) + ((t._ema,) if t._ema is not None else ())
    return [_np(b) for b in bufs]


def _grads(t):
    _settle(t)
    return _np(t.generator.grad_flat), _np(t.discriminator.grad_flat)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _row(l):
    return [float(l[k]) for k in LOSS_KEYS]


# ---------------------------------------------------------------------------------------------- 1. the kernel, bit for bit
def _call(lib, acc, g, n, mode, scale=1.0):
    rc = lib.pg_grad_accum(acc.ptr(), g.ptr(), n, mode, float(scale), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('n', A.NS + (ADAM_BIG_N,))
def test_kernel_bit_for_bit(n):
    """A k = 3 window (BEGIN, ADD, CLOSE with fl(1/3)) and a CLOSE_ONLY on mixed inputs in guarded buffers: the written operand has the
    replay's bits (NaN positions included), the operand the mode only reads keeps its bytes, the guards keep theirs."""
    lib = _lib()
    g1, g2, g3 = (A.mixed(n, 100 + i) for i in range(3))
    ACC = GU.flat(4 * n)
    G = GU.flat_from(torch.from_numpy(g1))

    def put(buf, values):
        buf.inner(torch.float32).copy_(torch.from_numpy(values))

    def got(buf):
        return buf.inner(torch.float32).cpu().numpy()
    # BEGIN: acc = g
    snap = G.snapshot()
    assert _call(lib, ACC, G, n, A.BEGIN) == 0
    want_acc, _ = A.replay(A.BEGIN, g1, g1)
    assert A.same_bits(got(ACC), want_acc), 'BEGIN'
    GU.assert_unchanged(G, snap, 'BEGIN g')
    GU.assert_untouched(ACC, 'all', 'BEGIN acc')
    # ADD: acc += g
    put(G, g2)
    snap = G.snapshot()
    assert _call(lib, ACC, G, n, A.ADD, NAN) == 0          # (the scale is not read in the first two modes)
    want_acc, _ = A.replay(A.ADD, want_acc, g2)
    assert A.same_bits(got(ACC), want_acc), 'ADD'
    GU.assert_unchanged(G, snap, 'ADD g')
    GU.assert_untouched(ACC, 'all', 'ADD acc')
    # CLOSE: g = (acc + g) * fl(1/3)
    put(G, g3)
    snap = ACC.snapshot()
    assert _call(lib, ACC, G, n, A.CLOSE, A.scale_of(3)) == 0
    _, want_g = A.replay(A.CLOSE, want_acc, g3, A.scale_of(3))
    assert A.same_bits(got(G), want_g), 'CLOSE'
    assert A.same_bits(want_g, A.window([g1, g2, g3])[1])
    GU.assert_unchanged(ACC, snap, 'CLOSE acc')
    GU.assert_untouched(G, 'all', 'CLOSE g')
    # CLOSE_ONLY: g = acc * fl(1/2), whatever g held
    G.inner().fill_(GU.SENTINEL)
    assert _call(lib, ACC, G, n, A.CLOSE_ONLY, A.scale_of(2)) == 0
    _, want_g = A.replay(A.CLOSE_ONLY, want_acc, g3, A.scale_of(2))
    assert A.same_bits(got(G), want_g), 'CLOSE_ONLY'
    GU.assert_unchanged(ACC, snap, 'CLOSE_ONLY acc')
    GU.assert_untouched(G, 'all', 'CLOSE_ONLY g')
    if n >= 64:
        nan = np.isnan(want_g)
        assert nan.any() and not nan.all() and np.isinf(want_g).any()


# ---------------------------------------------------------------------------------------------- 2. PG_EINVAL touches nothing
def test_einval_touches_nothing():
    lib = _lib()
    n = 1023
    acc = torch.from_numpy(A.mixed(n, 1)).to(DEV)
    both = torch.from_numpy(A.mixed(2 * n + 8, 2)).to(DEV)          # g, and room behind it for the overlapping cases
    g = both[:n]
    before = [acc.clone(), both.clone()]
    Ap, Gp = acc.data_ptr(), g.data_ptr()
    assert Ap % 16 == 0 and Gp % 16 == 0

    def call(a=Ap, g=Gp, n=n, mode=A.CLOSE, scale=0.5):
        return lib.pg_grad_accum(a, g, n, mode, scale, None)
    for mode in (A.BEGIN, A.ADD, A.CLOSE, A.CLOSE_ONLY):
        assert call(a=None, mode=mode) == -1 and call(g=None, mode=mode) == -1
        assert call(a=Ap + 4, mode=mode) == -1 and call(g=Gp + 8, mode=mode) == -1
        assert call(n=0, mode=mode) == -1 and call(n=-1, mode=mode) == -1
        assert call(a=Gp, mode=mode) == -1 and call(a=Gp + 16, mode=mode) == -1 and call(a=Gp + 4 * (n - 3), mode=mode) == -1
    for mode in (-1, 4):
        assert call(mode=mode) == -1
    for mode in (A.CLOSE, A.CLOSE_ONLY):
        for bad in (NAN, INF, -INF, 0.0, -0.5, 1.0000001, 2.0):
            assert call(mode=mode, scale=bad) == -1, (mode, bad)
    torch.cuda.synchronize()
    for a, b in zip((acc, both), before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # (and the same arguments un-spoilt are accepted: ranges that touch without intersecting, a scale of 1)
    assert call(a=Gp + 4 * (n + 1), mode=A.BEGIN) == 0 and call(mode=A.CLOSE, scale=1.0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. two identical micro-batches are one plain step
def test_two_identical_micro_batches_are_one_plain_step(tmp_path):
    """(g + g) * 0.5f == g in fp32: with accumulate = 2 two calls on the same (x, y) leave weights, moments, the weight average and
    the step counts exactly where ONE step of a trainer without the feature leaves them; after the first call nothing has moved.  (Only
    k = 2 has this identity: 3 g already rounds.)  Fails without the feature: two calls are then two updates."""
    (x, y), = _batches(1)
    plain = _trainer(tmp_path / 'plain', ema_decay=0.99)
    first = _state(plain)
    want_loss = _row(plain.batch(x, y, train=True))
    want = _state(plain)
    assert (plain._t_g, plain._t_d) == (1, 1) and plain._acc is None
    t = _trainer(tmp_path / 'acc', accumulate=2, ema_decay=0.99)
    assert _same(_state(t), first)
    l1 = _row(t.batch(x, y, train=True))
    assert _same(_state(t), first) and (t._t_g, t._t_d) == (0, 0)          # weights, moments and the average: their initial bits
    l2 = _row(t.batch(x, y, train=True))
    assert l1 == want_loss and l2 == want_loss                               # each call returns its own micro-batch's losses
    assert (t._t_g, t._t_d) == (1, 1)
    got = _state(t)
    assert len(got) == 7 and _same(got, want)
    assert not _same(got[:2], first[:2])


# ---------------------------------------------------------------------------------------------- 4. a k = 3 window of different micro-batches
def test_window_of_three_is_the_replay_of_its_gradients(tmp_path):
    data = _batches(3)
    t = _trainer(tmp_path / 'acc', accumulate=3)
    first = _state(t)
    t.batch(*data[0], train=True)
    g1 = _grads(t)
    t.batch(*data[1], train=True)
    g2 = _grads(t)
    assert _same(_state(t), first) and (t._t_g, t._t_d) == (0, 0)            # the weights have not moved
    for i in (0, 1):
        assert A.same_bits(_np(t._acc[i]), A.replay(A.ADD, g1[i], g2[i])[0])  # both accumulators are g1 + g2
    twin = _trainer(tmp_path / 'twin')                                       # (x3, y3) as the first step from the same initial weights
    twin.batch(*data[2], train=True)
    g3 = _grads(twin)
    t.batch(*data[2], train=True)
    closed = _grads(t)
    assert (t._t_g, t._t_d) == (1, 1)
    got = _state(t)
    for i, name in enumerate(('gen', 'disc')):
        want = A.window([g1[i], g2[i], g3[i]])[1]
        assert np.isfinite(want).all() and np.abs(want).sum() > 0
        assert A.same_bits(closed[i], want), name
        p0, m0, v0 = (torch.from_numpy(first[j]).double() for j in (i, 2 + 2 * i, 3 + 2 * i))
        mine = tuple(torch.from_numpy(got[j]) for j in (i, 2 + 2 * i, 3 + 2 * i))
        r = U.adamw_ratios(mine, (p0, torch.from_numpy(want).double(), m0, v0), U.scalars(1, LRS[i], 0.9, 0.999), None)
        print(f'k=3 window, {name}: step-1 ratios on the closed gradient {r}')
        assert all(val <= 1.0 for val in r.values()), (name, r)
        assert not np.array_equal(got[i], first[i])
    for x, y in data:
        t.batch(x, y, train=True)
    _settle(t)
    assert (t._t_g, t._t_d) == (2, 2)


# ---------------------------------------------------------------------------------------------- 5. the window is the large batch where the loss is a mean
def test_window_is_the_large_batch_for_a_mean_loss(tmp_path):
    """loss_type = 'MAE', one output channel, InstanceNorm, dropout off: accumulate = 2 over the two halves of a batch of four against a
    trainer without the feature on the whole batch.  The bound is the one tests/test_dp_gpu.py holds the same comparison of summation
    orders to (it measured 8e-8 .. 7e-7 there): relative L2 < 1e-5, norm ratio within 1e-5 of 1, losses to 1e-6."""
    (x, y), = _batches(1, seed=8, B=4)
    big = _trainer(tmp_path / 'big', loss_type='MAE')
    want_loss = np.array(_row(big.batch(x, y, train=True)))
    want = _grads(big)
    t = _trainer(tmp_path / 'acc', accumulate=2, loss_type='MAE')
    rows = np.array([_row(t.batch(x[:2], y[:2], train=True)), _row(t.batch(x[2:], y[2:], train=True))])
    got = _grads(t)
    for name, a, b in (('G', got[0], want[0]), ('D', got[1], want[1])):
        a, b = a.astype(np.float64), b.astype(np.float64)
        rel, ratio = np.linalg.norm(a - b) / np.linalg.norm(b), np.linalg.norm(a) / np.linalg.norm(b)
        print(f'window of two halves vs the batch of four, {name} gradient: relative L2 {rel:.2e}, norm ratio {ratio:.7f}')
        assert rel < 1e-5 and abs(ratio - 1) < 1e-5, (name, rel, ratio)
    err = np.abs(rows.mean(axis=0) - want_loss) / np.maximum(np.abs(want_loss), 1e-6)
    print(f'mean of the two calls losses vs the large batch: relative error {err}')
    assert err.max() < 1e-6, err
    assert (t._t_g, t._t_d) == (1, 1) == (big._t_g, big._t_d)


# ---------------------------------------------------------------------------------------------- 6. launch modes
def _run(folder, accumulate=2, calls=12, **kw):
    t = _trainer(folder, accumulate=accumulate, nf=16, **kw)
    rows, used = [], []
    for x, y in _batches(calls):
        rows.append(_row(t.batch(x, y, train=True)))
        used.append(t.launch_mode)
    return np.array(rows), _state(t), used, t


def test_launch_modes_give_the_same_bits(tmp_path):
    one = _run(tmp_path / 'one')
    assert set(one[2]) == {'eager1'}
    two = _run(tmp_path / 'two', two_streams=True)
    assert set(two[2]) == {'eager2'}
    rep = _run(tmp_path / 'graph', graph=True)
    # three warm calls per phase, then each phase replays its own graph; only the closing one holds Adam
    assert rep[2] == ['eager1'] * 6 + ['graph'] * 6, rep[2]
    phases = sorted(key[0][-1][2] for key in rep[3]._graphs)
    assert phases == ['begin', 'close'], phases
    assert all(key[0][-1][:2] == ('accum', 2) for key in rep[3]._graphs)
    for other in (two, rep):
        assert np.array_equal(one[0], other[0])
        assert _same(one[1], other[1])
        assert other[3]._t_g == other[3]._t_d == 6
    assert one[3]._t_g == one[3]._t_d == 6
    # (the setting took effect: a trainer without it ends elsewhere, twelve updates on)
    plain = _run(tmp_path / 'plain', accumulate=None)
    assert plain[3]._t_g == 12 and not np.array_equal(one[1][0], plain[1][0]) and not np.array_equal(one[1][1], plain[1][1])


# ---------------------------------------------------------------------------------------------- 7. everything on at once
def test_every_option_at_once(tmp_path):
    """Spectral D, clipping, the weight average, betas, a decay and accumulate = 2 over two windows: each closing call is the float64
    AdamW step (tests/test_optim_gpu.py's check) on grad_flat -- the closed, mapped gradient -- times the read-back coefficient; the
    non-closing calls leave everything, the average included, alone; the status blocks count updates, not calls."""
    betas, wds = ((0.5, 0.999), (0.0, 0.9)), (1e-2, None)
    t = _trainer(tmp_path, accumulate=2, spectral=True, clip_grad_norm=(1.0, 1.0), ema_decay=0.99, betas=betas, weight_decay=wds)
    g, d = t.generator, t.discriminator
    nets = (('gen', g, 0, wds[0]), ('disc', d, 2, wds[1]))
    for call, (x, y) in enumerate(_batches(4), 1):
        before = _state(t)
        t.batch(x, y, train=True)
        after = _state(t)
        if call % 2:
            assert _same(after, before) and (t._t_g, t._t_d) == (call // 2, call // 2), call
            continue
        step = call // 2
        assert (t._t_g, t._t_d) == (step, step)
        stats = t.read_grad_stats()
        for (name, net, i, wd), lr, (b1, b2) in zip(nets, LRS, betas):
            j = 0 if name == 'gen' else 1
            p, m, v = (torch.from_numpy(before[k]).double() for k in (j, 2 + i, 3 + i))
            assert stats[name]['steps'] == step and stats[name]['skipped'] == 0 and 0.0 < stats[name]['coef'] <= 1.0
            grad = scaled(net.grad_flat.double().cpu(), stats[name]['coef'])
            got = tuple(torch.from_numpy(after[k]) for k in (j, 2 + i, 3 + i))
            dm = U.decay_mul(lr, wd) if wd is not None else None
            r = U.adamw_ratios(got, (p, grad, m, v), U.scalars(step, lr, b1, b2), dm)
            print(f'window {step} {name}: {r}')
            assert all(val <= 1.0 for val in r.values()), (step, name, r)
            assert bool(grad.abs().sum() > 0) and not torch.equal(got[0].double(), p)
        c = float(np.float32(1.0) - np.float32(0.99))
        assert U.ema_ratio(torch.from_numpy(after[6]), torch.from_numpy(before[6]).double(), torch.from_numpy(after[0]), c) <= 1.0
        assert not np.array_equal(after[6], before[6])
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['disc']['steps'] == 2


# ---------------------------------------------------------------------------------------------- 8. a NaN skips the window
def test_a_nan_in_one_micro_batch_skips_the_windows_update(tmp_path):
    data = _batches(4)
    bad_x = data[0][0].clone()
    bad_x[0, 1, 17, 33] = NAN
    t = _trainer(tmp_path, accumulate=2, clip_grad_norm=(1.0, 1.0), ema_decay=0.99)
    first = _state(t)
    t.batch(bad_x, data[0][1], train=True)
    t.batch(*data[1], train=True)
    assert _same(_state(t), first)                                           # all state bits kept
    stats = t.read_grad_stats()
    for name in ('gen', 'disc'):
        assert stats[name]['steps'] == 1 and stats[name]['skipped'] == 1, (name, stats[name])
    assert np.isnan(_grads(t)[0]).any() and np.isnan(_grads(t)[1]).any()     # the NaN reached the closed gradient of either network
    t.batch(*data[2], train=True)
    t.batch(*data[3], train=True)
    after = _state(t)
    stats = t.read_grad_stats()
    for name in ('gen', 'disc'):
        assert stats[name]['steps'] == 2 and stats[name]['skipped'] == 1 and np.isfinite(stats[name]['norm']), (name, stats[name])
    assert all(np.isfinite(b).all() for b in after)
    assert all(not np.array_equal(a, b) for a, b in zip(after, first))       # the next window updates normally


# ---------------------------------------------------------------------------------------------- 9. short windows and discards
def test_step_accumulated_closes_a_short_window(tmp_path):
    data = _batches(2)
    t = _trainer(tmp_path, accumulate=3)
    first = _state(t)
    t.batch(*data[0], train=True)
    g1 = _grads(t)
    t.batch(*data[1], train=True)
    g2 = _grads(t)
    assert t.step_accumulated() is True
    closed = _grads(t)
    for i in (0, 1):
        assert A.same_bits(closed[i], A.window([g1[i], g2[i]], short=True)[1])          # (g1 + g2) * fl(1/2)
    assert (t._t_g, t._t_d) == (1, 1)
    after = _state(t)
    assert all(not np.array_equal(a, b) for a, b in zip(after, first))
    assert t.step_accumulated() is False                                      # called again, it does nothing
    assert _same(_state(t), after) and (t._t_g, t._t_d) == (1, 1)
    t.accumulate = None
    assert t.step_accumulated() is False


def test_train_closes_the_last_window_of_an_epoch(tmp_path, capsys):
    t = _trainer(tmp_path, accumulate=2)
    t.train(_batches(5), [], epochs=1, save_freq=10)
    _settle(t)
    assert (t._t_g, t._t_d) == (3, 3) and t._acc_done == 0                    # 2 + 2 + 1 micro-batches: three updates
    assert 'Accumulation -- 3 optimizer steps from 5 micro-batches' in capsys.readouterr().out


@pytest.mark.parametrize('how', ['setup_optimizers', 'load'])
def test_a_discarded_window_starts_over(tmp_path, how):
    data = _batches(2)
    t = _trainer(tmp_path, accumulate=3)
    if how == 'load':
        t.save(1)
    t.batch(*data[0], train=True)
    assert t._acc_done == 1
    if how == 'load':
        t.load(f'{t.savefolder}/generator_ep_001.pth', f'{t.savefolder}/discriminator_ep_001.pth')
    else:
        t.setup_optimizers(*LRS)
    assert t._acc_done == 0
    t.batch(*data[1], train=True)
    g2 = _grads(t)
    assert t._acc_done == 1 and (t._t_g, t._t_d) == (0, 0)
    for i in (0, 1):
        assert A.same_bits(_np(t._acc[i]), g2[i])                             # that call's gradient alone


# ---------------------------------------------------------------------------------------------- 10. off is off
@pytest.mark.parametrize('off', [None, 1])
def test_default_trainer_keeps_its_kind_key_and_calls(tmp_path, monkeypatch, off):
    from patchgan_amd import _lib as L, engine as E
    real = L.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith('pg_adam') or name == 'pg_grad_accum':
                calls.append(name)
            return getattr(real, name)
    t = _trainer(tmp_path, accumulate=off, nf=16, graph=True)
    (x, y), = _batches(1)
    monkeypatch.setattr(E.L, 'load', lambda: Spy())
    for _ in range(5):
        t.batch(x, y, train=True)
    _settle(t)
    monkeypatch.undo()
    assert calls == ['pg_adam_step'] * 6 + ['pg_adam_step_dev'] * 2, calls          # three eager steps and the capture, as ever
    c = Golden(GOLD).cfg
    dims = (c['B'], c['size'], c['size'], c['in_nc'], c['out_nc'])
    xd, yd = x.cuda(), y.cuda()
    assert t._kind_key(xd, yd, False, dims, True) == t._kind_key_base(xd, yd, False, dims, True) and t._acc_key() == ()
    assert t._acc is None and t._acc_done == 0 and t._acc_launches == 0 and (t._t_g, t._t_d) == (5, 5)
    assert len(t._graphs) == 1 and len(next(iter(t._graphs.values())).ptrs) == 10


# ---------------------------------------------------------------------------------------------- 11. data parallel
def _worker(rank, world, port, q, gw, dw, data):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    import patchgan_amd as pg
    from patchgan_amd.parallel import shard_batch
    c = Golden(GOLD).cfg
    g = pg.UNet(c['in_nc'], c['out_nc'], c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], c['ndf'], n_layers=c['n_layers'], norm=c['norm'])
    g.load_state_dict(gw)
    d.load_state_dict(dw)
    g.cuda(), d.cuda()
    g.train(), d.train()
    t = pg.Trainer(g, d, tempfile.mkdtemp())
    t.accumulate = 2
    t.bucket_bytes = 64 << 10          # several buckets even for the nf=4 generator
    t.setup_optimizers(*LRS)
    rows, closed = [], None
    for i, (x, y) in enumerate(data):
        xs, ys = shard_batch(x, y, rank, world)
        rows.append(_row(t.batch(xs, ys, train=True)))
        if i == 1:
            closed = _grads(t)          # window 1's closed gradients (D's update is applied by the flush in there)
    state = _state(t)
    q.put((rank, np.array(rows), state, closed, (t._t_g, t._t_d)))
    dist.destroy_process_group()


def test_two_ranks_accumulate_what_the_single_process_does(tmp_path):
    """Two gloo ranks on the one GPU, one sample each, accumulate = 2, against the single process with accumulate = 2 on the unsharded
    micro-batches: every call's gradients are all-reduced as without the feature and the REDUCED gradient is accumulated.  The bounds
    are those of tests/test_dp_gpu.py."""
    from tests.test_dp_gpu import _collect
    data = _batches(4)
    t = _trainer(tmp_path / 'single', accumulate=2)
    gw = {k: v.detach().cpu().clone() for k, v in t.generator.state_dict().items()}
    dw = {k: v.detach().cpu().clone() for k, v in t.discriminator.state_dict().items()}
    single, want = [], None
    for i, (x, y) in enumerate(data):
        single.append(_row(t.batch(x, y, train=True)))
        if i == 1:
            want = _grads(t)
    single = np.array(single)
    _settle(t)
    assert (t._t_g, t._t_d) == (2, 2)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, gw, dw, data)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, s0, g0, n0), (_, c1, s1, g1, n1) = res
    assert _same(s0, s1) and _same(g0, g1) and n0 == n1 == (2, 2)            # the ranks are bit-identical to each other
    assert np.allclose(c0, c1, rtol=1e-6)
    for name, got, ref in (('G', g0[0], want[0]), ('D', g0[1], want[1])):
        rel = np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref.astype(np.float64))
        print(f'dp2 accumulate=2, window-1 closed {name} gradient vs single process: relative L2 {rel:.2e}')
        assert rel < 1e-5, (name, rel)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('dp2 accumulate=2 vs single process: max rel err per call', err.max(axis=1))
    assert err[:2].max() < 1e-6, err
    assert err.max() < 1e-4, err
