"""Differentiable augmentation of the discriminator's inputs on the GPU (Trainer.diffaug; diffaug.hip): the parameter kernel against the
Python restatement (exact), the map and its adjoint against NumPy (bit for bit, between guards), the generator's gradient through D o T
against the float64 oracle, a three-step training curve, the launch modes, off-is-off, data parallelism and the smoke checks.
Needs an MI355X."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import diffaug_util as U
from tests import guard_util as GU
from tests.golden_util import Golden, LOSS_KEYS

pytestmark = pytest.mark.gpu

ALL = 'flip,translation,cutout'
EINVAL = -1


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- A. the parameter kernel
def _table(seed, counter, step, policy, sample0, N, H, W):
    """One pg_diffaug_params call into a guarded table.  counter: a guarded 8-byte word or None.  -> int32 [N, 8]."""
    g = GU.flat(N * 32)
    rc = _lib().pg_diffaug_params(seed, counter.ptr() if counter is not None else None, step, policy, sample0, N, H, W, g.ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    GU.assert_untouched(g, 'all', 'pg_diffaug_params table')
    return g.inner(torch.int32).cpu().numpy().reshape(N, 8).copy()


def _counter(t):
    c = GU.flat(8)
    c.inner(torch.int64).fill_(t)
    return c


def _count(c):
    return int(c.inner(torch.int64).item())


@pytest.mark.parametrize('sample0', [0, 3])
@pytest.mark.parametrize('H,W', [(8, 12), (256, 256)])
def test_params_equal_the_restatement(H, W, sample0):
    N, seed = 5, 0x123456789ABCDEF1
    for policy in U.POLICIES:
        c = _counter(41)
        got = _table(seed, c, 999, policy, sample0, N, H, W)           # (the host step is ignored when there is a counter)
        assert np.array_equal(got, U.params_ref(seed, 41, policy, sample0, N, H, W)), (policy, got)
        GU.assert_untouched(c, 8, 'counter')
        assert _count(c) == 42                                         # advanced by exactly one
        assert np.array_equal(_table(seed, c, 0, policy, sample0, N, H, W), U.params_ref(seed, 42, policy, sample0, N, H, W))
        assert _count(c) == 43
        assert np.array_equal(_table(seed, None, 41, policy, sample0, N, H, W), got)          # the host-step path, the same t


def test_params_split_into_two_calls_and_many_samples():
    seed, H, W = 77, 256, 256
    whole = _table(seed, None, 6, 7, 0, 5, H, W)
    parts = np.concatenate([_table(seed, None, 6, 7, 0, 2, H, W), _table(seed, None, 6, 7, 2, 3, H, W)])
    assert np.array_equal(whole, parts) and np.array_equal(whole, U.params_ref(seed, 6, 7, 0, 5, H, W))
    # more samples than the workgroup has lanes: the strided loop, and the counter still advances once
    c = _counter(0)
    big = _table(seed, c, 0, 7, 10, 600, 16, 24)
    assert np.array_equal(big, U.params_ref(seed, 0, 7, 10, 600, 16, 24)) and _count(c) == 1


def test_params_argument_errors_write_nothing():
    g, c = GU.flat(5 * 32), _counter(3)
    snap = c.snapshot()
    lib = _lib()
    for args in ((0, c.ptr(), 0, 7, 0, 5, 8, 8, None), (0, c.ptr() + 4, 0, 7, 0, 5, 8, 8, g.ptr()), (0, c.ptr(), 0, 8, 0, 5, 8, 8, g.ptr()),
                 (0, c.ptr(), 0, 7, -1, 5, 8, 8, g.ptr()), (0, c.ptr(), 0, 7, 0, 0, 8, 8, g.ptr()), (0, c.ptr(), 0, 7, 0, 5, 0, 8, g.ptr())):
        assert lib.pg_diffaug_params(*args, _stream()) == EINVAL, args
    torch.cuda.synchronize()
    GU.assert_untouched(g, None, 'table')
    GU.assert_unchanged(c, snap, 'counter')


# ---------------------------------------------------------------------------------------------- B. the map and its adjoint
def _layouts(C):
    out = [('dense', C, 0), ('slice1', 8 if C < 8 else 16, 1)]          # channel offset 1: the scalar form
    if C % 4 == 0:
        out.append(('slice4', C + 4, 4))                                 # a 16-byte-aligned slice: the 16-byte form on ld > C
    return out


CASES = [(H, W, C, name, ld, off) for H, W in ((8, 12), (16, 24), (33, 20)) for C in (1, 4, 5, 8) for name, ld, off in _layouts(C)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _read(v, off):
    return v.t[:v.npix * v.ld].view(v.N, v.H, v.W, v.ld)[..., off:off + v.C].cpu().numpy()


@pytest.mark.parametrize('H,W,C,name,ld,off', CASES, ids=[f'{h}x{w}-C{c}-{n}' for h, w, c, n, _, _ in CASES])
def test_fwd_and_bwd_equal_numpy_bit_for_bit(H, W, C, name, ld, off):
    N = 3
    lib = _lib()
    rng = np.random.default_rng(H * 1000 + W * 10 + C)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    x[0, 0, 0, 0], x[-1, -1, -1, -1] = -0.0, np.float32(1e-42)          # a negative zero and a denormal travel as bits
    src, src_g = GU.view_from(torch.from_numpy(x).permute(0, 3, 1, 2), ld, off)
    vec = C % 4 == 0 and ld % 4 == 0 and src.ptr() % 16 == 0
    assert vec == (C % 4 == 0 and name != 'slice1')                      # both forms are reached by the cases
    ins = GU.Inputs()
    ins.add(src_g, 'src')
    for policy in U.POLICIES:
        from_kernel = _table(1000 + policy, None, 2, policy, 0, N, H, W)
        for table in [from_kernel] + [U.masked(t, policy) for t in U.extreme_tables(N, H, W)]:
            tab_g = GU.flat_from(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)))
            ins.add(tab_g, 'table')
            for fn, ref in ((lib.pg_diffaug_fwd, U.apply), (lib.pg_diffaug_bwd, U.adjoint)):
                dst, dst_g = GU.view(N, H, W, C, ld, off)
                assert fn(src.ptr(), src.ld, dst.ptr(), dst.ld, tab_g.ptr(), N, H, W, C, _stream()) == 0
                torch.cuda.synchronize()
                GU.assert_untouched(dst_g, 'slice', f'{fn.__name__} dst')
                got, want = _read(dst, off), ref(x, table)
                assert np.array_equal(_bits(got), _bits(want)), (fn.__name__, policy, table)
    ins.check('pg_diffaug')


def test_move_argument_errors_write_nothing():
    N, H, W, C = 2, 8, 12, 4
    lib = _lib()
    src, src_g = GU.view_from(torch.zeros(N, C, H, W))
    dst, dst_g = GU.view(N, H, W, C)
    wide, wide_g = GU.view(N, H, W, 8)
    tab_g = GU.flat_from(torch.zeros(N, 8, dtype=torch.int32))
    for fn in (lib.pg_diffaug_fwd, lib.pg_diffaug_bwd):
        assert fn(None, 4, dst.ptr(), 4, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL
        assert fn(src.ptr(), 4, None, 4, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL
        assert fn(src.ptr(), 4, dst.ptr(), 4, None, N, H, W, C, _stream()) == EINVAL
        assert fn(src.ptr(), 3, dst.ptr(), 4, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL          # ld < C
        assert fn(src.ptr(), 4, dst.ptr(), 3, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL
        assert fn(dst.ptr(), 4, dst.ptr(), 4, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL          # in place
        # two channel slices of one buffer: the ranges intersect
        assert fn(wide.ptr(), 8, wide.ptr() + 16, 8, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL
        assert fn(wide.ptr() + 16, 8, wide.ptr(), 8, tab_g.ptr(), N, H, W, C, _stream()) == EINVAL
    torch.cuda.synchronize()
    GU.assert_untouched(dst_g, None, 'dst')
    GU.assert_untouched(wide_g, None, 'wide')


# ---------------------------------------------------------------------------------------------- C. the trainer
def _nets(gold=None, nf=None, ndf=None, **dkw):
    """a_lrelu_tversky's networks with the fixture's weights; another width or discriminator option: torch's initialisation."""
    import patchgan_amd as pg
    gold = gold or Golden('a_lrelu_tversky')
    c = gold.cfg
    g = pg.UNet(c['in_nc'], c['out_nc'], nf or c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], ndf or c['ndf'], n_layers=c['n_layers'], norm=dkw.pop('norm', c['norm']), **dkw)
    if nf is None:
        g.load_state_dict(gold.weights('g0'))
    if ndf is None and not dkw:
        d.load_state_dict(gold.weights('d0'))
    return g.cuda(), d.cuda()


def _trainer(g, d, folder, mode=None, **attrs):
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(folder))
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers(1e-3, 1e-3)
    if mode is not None:
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    g.train()
    d.train()
    return t


def _oracle(gold, dtype, **kw):
    c = gold.cfg
    args = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=c['loss_type'], dtype=dtype)
    args.update(kw)
    return U.AugOracleTrainer(gold.weights('g0'), gold.weights('d0'), **args)


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def test_generator_gradient_through_the_adjoint(tmp_path):
    """seg_alpha = 0 with the MAE loss: the generator's gradient arrives ONLY through D o T, so a missing or wrong adjoint shows in every
    parameter.  Every generator parameter's .grad after one training step against AugOracleTrainer(float64) with the table read
    back; metric and bound of tests/test_configs_gpu.py for the same comparison without the option: relative L2 < 2e-2 and
    <= 8 x noise + 1e-3, noise the fp32 oracle's own relative-L2 distance from float64.  Against the float64 oracle WITHOUT the
    augmentation the whole gradient must lie at least 10 x the largest of those bounds away: the test can see the map (measured on an
    MI355X: 1.06 in relative L2 -- all but unrelated vectors --, 1017 x the largest bound; 1.5e-06 from the oracle with the map)."""
    gold = Golden('a_lrelu_tversky')
    x, y = gold.inputs()
    N, _, H, W = x.shape
    assert (N, H, W) == (2, 256, 256) and (gold.cfg['nf'], gold.cfg['ndf']) == (4, 4)
    seed = U.find_seed(N, H, W)
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=seed, loss_type='MAE', seg_alpha=0)
    t.batch(x, y, train=True)
    table = t.read_diffaug_params()
    assert np.array_equal(table, U.params_ref(seed, 0, 7, 0, N, H, W))
    assert all(U.interesting(r, H, W) for r in table), table
    got = {k: v.grad.detach().cpu() for k, v in g.named_parameters()}
    refs = {}
    for name, dtype, tab in (('o64', torch.float64, table), ('o32', torch.float32, table), ('plain64', torch.float64, None)):
        o = _oracle(gold, dtype, loss_type='MAE', seg_alpha=0)
        o.table = tab
        o.batch(x, y, train=True)
        refs[name] = o.last['g_grads']
    worst = 0.0
    for k, want in refs['o64'].items():
        e, noise = _l2(got[k], want), _l2(refs['o32'][k], want)
        print(f'diffaug G grad {k:40s} error {e:.2e} fp32-oracle noise {noise:.2e}')
        assert e < 2e-2 and e <= 8 * noise + 1e-3, (k, e, noise)
        worst = max(worst, 8 * noise + 1e-3)
    flat = lambda d_: torch.cat([d_[k].double().reshape(-1) for k in refs['o64']])
    far, near = _l2(flat(got), flat(refs['plain64'])), _l2(flat(got), flat(refs['o64']))
    print(f'diffaug G grad: distance from the float64 oracle {near:.2e}, from the float64 oracle WITHOUT augmentation {far:.2e} '
          f'= {far / worst:.1f} x the largest bound')
    assert far >= 10 * worst, (far, worst)
    t.release()


# The distance of a run from AugOracleTrainer(float64) on the same run (seed CURVE_SEED, the tables of step counts 0, 1, 2) is ONE number:
# the largest relative error among everything compared -- each of the 18 loss scalars relative to its own value, each parameter
# tensor of both networks after the third step in relative max-norm.  AugOracleTrainer(float32) lies 4.944e-04 from it (computed on
# the CPU; the largest term is a weight tensor, the losses alone are at 1.1e-07); the bound is 3 x that, the factor the yardstick of
# tests/test_step_gpu.py grants the reference's own fp32 noise.
CURVE_SEED = 5
CURVE_BOUND = 3 * 4.944e-04


def _curve_dist(curve, want, weights, want_w):
    e_l = float((np.abs(curve - want) / np.maximum(np.abs(want), 1e-6)).max())
    e_w = max(float((weights[k].double().cpu() - w.double()).abs().max() / w.double().abs().max()) for k, w in want_w.items())
    return e_l, e_w


def test_three_step_curve_against_the_float64_oracle(tmp_path):
    """Three training steps of a_lrelu_tversky's networks with all three policies: the six losses of every step and the final weights
    of both networks against AugOracleTrainer(float64) fed with the tables read back (measured on an MI355X: 6.79e-04, the weights;
    the losses alone 4.7e-07)."""
    gold = Golden('a_lrelu_tversky')
    x, y = gold.inputs()
    N, _, H, W = x.shape
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=CURVE_SEED, loss_type=gold.cfg['loss_type'])
    o64 = _oracle(gold, torch.float64)
    curve, want = [], []
    for s in range(3):
        l = t.batch(x, y, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
        o64.table = t.read_diffaug_params()
        assert np.array_equal(o64.table, U.params_ref(CURVE_SEED, s, 7, 0, N, H, W))
        w = o64.batch(x, y, train=True)
        want.append([w[k] for k in LOSS_KEYS])
    t.flush()
    got_w = {**{'g.' + k: v for k, v in g.state_dict().items()}, **{'d.' + k: v for k, v in d.state_dict().items()}}
    want_w = {**{'g.' + k: v.detach() for k, v in o64.gw.items()}, **{'d.' + k: v.detach() for k, v in o64.dw.items()}}
    e_l, e_w = _curve_dist(np.array(curve), np.array(want), got_w, want_w)
    print(f'diffaug 3-step curve vs float64 oracle: losses {e_l:.3e}, weights {e_w:.3e}; distance {max(e_l, e_w):.3e}, bound {CURVE_BOUND:.3e}')
    assert max(e_l, e_w) <= CURVE_BOUND, (e_l, e_w)
    t.release()


STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3): three replays
MODE_SEED = 21
_MODE_RUNS = {}


def _mode_run(tmp_path_factory, mode):
    if mode not in _MODE_RUNS:
        g, d = _nets()
        x, y = Golden('a_lrelu_tversky').inputs()
        t = _trainer(g, d, tmp_path_factory.mktemp('aug_mode'), mode, diffaug=ALL, diffaug_seed=MODE_SEED)
        rows, modes, tables = [], [], []
        for s in range(STEPS):
            l = t.batch(x, y, train=True)
            rows.append([float(l[k]) for k in LOSS_KEYS])
            modes.append(t.launch_mode)
            tables.append(t.read_diffaug_params())
        t.flush()
        torch.cuda.synchronize()
        _MODE_RUNS[mode] = dict(losses=np.array(rows), modes=modes, tables=np.array(tables), g=g.flat.cpu().numpy().copy(),
                                d=d.flat.cpu().numpy().copy())
        t.release()
    return _MODE_RUNS[mode]


@pytest.mark.parametrize('mode', ['eager2', 'graph'])
def test_launch_modes_are_bit_identical(tmp_path_factory, mode):
    one, other = _mode_run(tmp_path_factory, 'eager1'), _mode_run(tmp_path_factory, mode)
    assert other['modes'][3:] == [mode] * (STEPS - 3) and one['modes'] == ['eager1'] * STEPS, (one['modes'], other['modes'])
    assert np.array_equal(one['losses'], other['losses']), one['losses'] - other['losses']
    assert np.array_equal(one['g'], other['g']) and np.array_equal(one['d'], other['d'])
    assert np.array_equal(one['tables'], other['tables'])
    assert np.isfinite(one['losses']).all()
    want = np.array([U.params_ref(MODE_SEED, s, 7, 0, 2, 256, 256) for s in range(STEPS)])
    assert np.array_equal(other['tables'], want)
    # the counter advances under replay: every step's table differs from every other's
    for i in range(STEPS):
        for j in range(i + 1, STEPS):
            assert not np.array_equal(other['tables'][i], other['tables'][j]), (i, j)


class _Recorder:
    """Stands in for the loaded library: records the name of every entry point reached, calls through."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith('pg_'):
            self.names.append(name)
        return fn


def test_off_is_off(tmp_path, monkeypatch):
    """diffaug = None and a trainer whose attribute was never set: the same bits over three steps, and no diffaug entry point -- the only
    way to a k_diffaug_* launch -- among the library calls of the off trainer (the on trainer, for control, reaches all three and
    otherwise the calls of the off trainer)."""
    from patchgan_amd import _lib as L
    x, y = Golden('a_lrelu_tversky').inputs()
    runs, calls = {}, {}
    for tag, attrs in (('never', {}), ('none', {'diffaug': None}), ('on', {'diffaug': 'cutout'})):
        g, d = _nets()
        t = _trainer(g, d, tmp_path / tag, **attrs)
        rec = _Recorder(L.load())
        monkeypatch.setattr(L, '_lib', rec)
        rows = [[float(l[k]) for k in LOSS_KEYS] for l in (t.batch(x, y, train=True) for _ in range(3))]
        t.flush()
        torch.cuda.synchronize()
        monkeypatch.undo()
        runs[tag] = (np.array(rows), g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy())
        calls[tag] = rec.names
        if tag != 'on':
            assert t._aug_counter is None and t._aug_params is None
        t.release()
    for a, b in zip(runs['never'], runs['none']):
        assert np.array_equal(a, b)
    assert calls['never'] == calls['none'] and len(calls['none']) > 100
    assert not any('diffaug' in n for n in calls['none'])
    assert [n for n in calls['on'] if 'diffaug' in n] == ['pg_diffaug_params', 'pg_diffaug_fwd', 'pg_diffaug_fwd', 'pg_diffaug_bwd'] * 3
    assert [n for n in calls['on'] if 'diffaug' not in n] == calls['none']
    assert not np.array_equal(runs['on'][0], runs['none'][0])


# ---------------------------------------------------------------------------------------------- D. data parallelism
DP_SEED = 33


def _dp_worker(rank, world, port, q, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    g, d = _nets()
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tempfile.mkdtemp(), diffaug=ALL, diffaug_seed=DP_SEED)
    xs, ys = shard_batch(x, y, rank, world)
    curve, tables = [], []
    for s in range(nsteps):
        l = t.batch(xs, ys, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
        tables.append(t.read_diffaug_params())
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, np.array(curve), np.array(tables), g.flat.cpu().numpy(), d.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_draw_the_rows_of_the_single_process(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    nsteps = 3
    g, d = _nets()
    x, y = Golden('a_lrelu_tversky').inputs()
    assert x.shape[0] == 2
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=DP_SEED)
    single, tables = [], []
    for s in range(nsteps):
        l = t.batch(x, y, train=True)
        single.append([l[k] for k in LOSS_KEYS])
        tables.append(t.read_diffaug_params())
    single, tables = np.array(single), np.array(tables)
    t.release()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, nsteps)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, t0, g0, d0), (_, c1, t1, g1, d1) = res
    assert t0.shape == t1.shape == (nsteps, 1, 8)
    assert np.array_equal(t0[:, 0], tables[:, 0]) and np.array_equal(t1[:, 0], tables[:, 1])          # rows 0 and 1, every step
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert np.allclose(c0, c1, rtol=1e-6)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('diffaug dp2 vs single process: max rel err per step', err.max(axis=1))
    assert err.max() < 1e-4, err          # (the bound of tests/test_dp_gpu.py for the same comparison without the option)


# ---------------------------------------------------------------------------------------------- E. smoke checks
SMOKE_SEED = 8


def _smoke(t, x, y, nsteps=2, t0=0):
    N, _, H, W = x.shape
    rows = []
    for s in range(nsteps):
        l = t.batch(x, y, train=True)
        rows.append([float(l[k]) for k in LOSS_KEYS])
        assert np.array_equal(t.read_diffaug_params(), U.params_ref(SMOKE_SEED, t0 + s, 7, 0, N, H, W)), s
    t.flush()
    torch.cuda.synchronize()
    assert np.isfinite(rows).all(), rows
    return np.array(rows)


def test_bf16_networks_run(tmp_path):
    torch.manual_seed(99)
    g, d = _nets(nf=16, ndf=32)
    g.set_precision('bf16')
    d.set_precision('bf16')
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=SMOKE_SEED)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all()
    t.release()


@pytest.mark.parametrize('kind', ['batchnorm', 'spectral'])
def test_other_discriminators_run(tmp_path, kind):
    from torch import nn
    torch.manual_seed(3)
    g, d = _nets(**(dict(norm=True, norm_layer=nn.BatchNorm2d) if kind == 'batchnorm' else dict(spectral_norm=True)))
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=SMOKE_SEED, two_streams=True)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all()
    t.release()


def test_evaluation_steps_leave_the_counter_alone(tmp_path):
    g, d = _nets()
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, diffaug=ALL, diffaug_seed=SMOKE_SEED)
    _smoke(t, x, y, 1)
    plain_g, plain_d = _nets()
    plain = _trainer(plain_g, plain_d, tmp_path / 'plain')
    plain_g.flat.copy_(g.flat)
    plain_d.flat.copy_(d.flat)
    ev, ev_plain = t.batch(x, y, train=False), plain.batch(x, y, train=False)
    assert [ev[k] for k in LOSS_KEYS] == [ev_plain[k] for k in LOSS_KEYS]          # an evaluation step never augments
    assert int(t._aug_counter.item()) == 1
    t.batch(x, y, train=False)
    _smoke(t, x, y, 2, t0=1)                                                       # the next training steps draw t = 1, 2
    assert int(t._aug_counter.item()) == 3
    t.release()
    plain.release()
