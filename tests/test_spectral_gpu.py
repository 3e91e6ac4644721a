"""Spectral normalisation of the discriminator on the GPU: pg_spectral_fwd / pg_spectral_bwd through ctypes against the float64
reference of tests/spectral_util.py (stage by stage on what the kernel stored, bit-reproducible, contained), the module against
torch.nn.utils.spectral_norm on the reference (tests/golden/sn_a_*.npz), the training step against the reference's step with one
power iteration per step (sn_b.npz), and the option in every launch mode, under data parallelism, bf16, clipping, checkpoints and
the command-line entry point."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests import guard_util as GU
from tests import spectral_util as S
from tests.golden_util import LOSS_KEYS, Golden

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FLOOR_F, FLOOR_W = 2e-5, 3e-5          # tests/test_bench_layers_gpu.py: forward / data gradient, weight gradient (relative max-norm)


# ---------------------------------------------------------------------------------------------- A. the kernels
GAP = 8          # floats between the weight blocks of the test's flat buffer (a bias block's place), a planted pattern


def _layout(shapes):
    offs, off = [], GAP
    for a, b in shapes:
        offs.append(off)
        off += 16 * a * b + GAP
    return offs, off


def _call_kernels(shapes, iterate, seed=0):
    """pg_spectral_fwd then pg_spectral_bwd over `shapes` in ONE batched call each, every buffer between guards.  Returns the per-layer
    inputs and stored results (CPU tensors) and the raw bytes of everything the calls wrote."""
    from patchgan_amd import _lib as L
    lib = L.load()
    offs, n = _layout(shapes)
    data = [S.layer_inputs(a, b, seed) for a, b in shapes]
    flat = torch.arange(n, dtype=torch.float32) * 0.5 + 3.0          # the gaps: a pattern that a scaled or skipped copy would change
    grad = -flat.clone()
    for (W, u, v, g), off in zip(data, offs):
        flat[off:off + W.numel()] = S.pack(W)
        grad[off:off + W.numel()] = S.pack(g)
    inputs = GU.Inputs()
    gflat = inputs.add(GU.flat_from(flat), 'flat')
    geff, ggrad = GU.flat(n * 4), GU.flat_from(grad)
    items = (L.SpectralItem * len(shapes))()
    bufs = []
    for it, (a, b), (W, u, v, g), off in zip(items, shapes, data, offs):
        gu, gv, gs = GU.flat_from(u), GU.flat_from(v), GU.flat(4)
        bufs.append((gu, gv, gs))
        it.W, it.w_hat, it.g_off = gflat.ptr() + 4 * off, geff.ptr() + 4 * off, off
        it.u, it.v, it.sigma, it.Cout, it.Cin, it.iterate = gu.ptr(), gv.ptr(), gs.ptr(), a, b, int(iterate)
    need = lib.pg_spectral_workspace_bytes(len(shapes), items)
    assert need > 0
    gws = GU.flat(need)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pg_spectral_fwd(len(shapes), items, gflat.ptr(), geff.ptr(), n, gws.ptr(), need, st) == 0
    torch.cuda.synchronize()
    fwd_inputs = GU.Inputs()
    for gu, gv, gs in bufs:
        for gb, name in ((gu, 'u'), (gv, 'v'), (gs, 'sigma')):
            fwd_inputs.add(gb, name)
    fwd_inputs.add(geff, 'w_hat')
    assert lib.pg_spectral_bwd(len(shapes), items, ggrad.ptr(), n, gws.ptr(), need, st) == 0
    torch.cuda.synchronize()
    inputs.check('pg_spectral_fwd / _bwd')
    fwd_inputs.check('pg_spectral_bwd')          # the backward pair only reads what the forward sequence left
    for g_, what in ((geff, 'eff'), (ggrad, 'grad'), (gws, 'workspace')):
        GU.assert_untouched(g_, 'all', what)
    for (gu, gv, gs), (a, b) in zip(bufs, shapes):
        GU.assert_untouched(gu, 4 * a, 'u')
        GU.assert_untouched(gv, 64 * b, 'v')
        GU.assert_untouched(gs, 4, 'sigma')
    eff, gr = geff.inner(torch.float32).cpu(), ggrad.inner(torch.float32).cpu()
    outside = torch.ones(n, dtype=torch.bool)
    results = []
    for (a, b), (W, u, v, g), off, (gu, gv, gs) in zip(shapes, data, offs, bufs):
        m = 16 * a * b
        outside[off:off + m] = False
        results.append(dict(W=W, u0=u, v0=v, g=g, got=dict(
            u=gu.inner(torch.float32).cpu(), v=gv.inner(torch.float32).cpu(), sigma=gs.inner(torch.float32).cpu()[0],
            w_hat=S.unpack(eff[off:off + m], a, b), dW=S.unpack(gr[off:off + m], a, b))))
    # everything between the blocks: copied bit for bit into eff, untouched in the gradient
    assert torch.equal(eff[outside], flat[outside]) and torch.equal(gr[outside], grad[outside])
    raw = b''.join(t.cpu().numpy().tobytes() for t in [geff.inner(), ggrad.inner()] + [x.inner() for bs in bufs for x in bs])
    return results, raw


@pytest.mark.parametrize('iterate', [True, False], ids=['iterate', 'fixed'])
@pytest.mark.parametrize('shapes', [S.KERNEL_SHAPES, [(40, 24)]], ids=['four-layers', 'one-layer'])
def test_kernels_against_float64_contained_and_reproducible(shapes, iterate):
    results, raw = _call_kernels(shapes, iterate)
    for (a, b), r in zip(shapes, results):
        ratios = S.stage_ratios(r['W'], r['u0'], r['v0'], r['got'], iterate, r['g'])
        print(f'spectral kernels {a}x{b} iterate={iterate}: error / bound', {k: round(v, 4) for k, v in ratios.items()})
        assert all(x <= 1.0 for x in ratios.values()), ((a, b), ratios)
        if iterate:
            assert not torch.equal(r['got']['u'], r['u0']) or a == 1
    assert _call_kernels(shapes, iterate)[1] == raw          # the same inputs: the same bits


def test_kernels_without_the_copy_touch_only_the_blocks():
    """flat == eff == NULL: no copy -- w_hat of a single layer written, the bytes around it keep the sentinel."""
    from patchgan_amd import _lib as L
    lib = L.load()
    a, b = 8, 5
    W, u, v, g = S.layer_inputs(a, b)
    gW, gu, gv, gs, gh = GU.flat_from(S.pack(W)), GU.flat_from(u), GU.flat_from(v), GU.flat(4), GU.flat(64 * a * b)
    items = (L.SpectralItem * 1)()
    it = items[0]
    it.W, it.w_hat, it.u, it.v, it.sigma, it.Cout, it.Cin, it.iterate = gW.ptr(), gh.ptr(), gu.ptr(), gv.ptr(), gs.ptr(), a, b, 1
    need = lib.pg_spectral_workspace_bytes(1, items)
    gws = GU.flat(need)
    snap = gW.snapshot()
    assert lib.pg_spectral_fwd(1, items, None, None, 0, gws.ptr(), need, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    GU.assert_unchanged(gW, snap, 'W')
    for g_, nb in ((gh, 'all'), (gu, 4 * a), (gv, 64 * b), (gs, 4), (gws, 'all')):
        GU.assert_untouched(g_, nb, 'pg_spectral_fwd without copy')
    got = dict(u=gu.inner(torch.float32).cpu(), v=gv.inner(torch.float32).cpu(), sigma=gs.inner(torch.float32).cpu()[0],
               w_hat=S.unpack(gh.inner(torch.float32).cpu(), a, b))
    assert all(x <= 1.0 for x in S.stage_ratios(W, u, v, got, True).values())


# ---------------------------------------------------------------------------------------------- B. the module against torch
def _bound(fix32, fix64, floor):
    return max(2.0 * S.rel_dist(fix32, fix64), floor)


@pytest.mark.parametrize('name,norm', [('sn_a_plain', False), ('sn_a_norm', True)])
def test_module_against_torch_spectral_norm(name, norm):
    import patchgan_amd as pg
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    d = pg.Discriminator(5, 8, n_layers=3, norm=norm, spectral_norm=True)
    d.load_state_dict({k: torch.from_numpy(z['sd0/' + k].copy()) for k in z['keys']})
    d.cuda().train()
    x = torch.from_numpy(z['x'].copy()).cuda().requires_grad_(True)
    y = d(x)
    y.backward(torch.from_numpy(z['gout'].copy()).cuda())
    bad = []

    def check(what, got, floor):
        got = S.sample(got)          # (the elements the fixture stores: all of them up to 4096)
        err, bound = S.rel_dist(got, z[what + '64']), _bound(z[what + '32'], z[what + '64'], floor)
        print(f'{name} {what}: error {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append((what, err, bound))
    check('out', y.detach().cpu(), FLOOR_F)
    check('dx', x.grad.cpu(), FLOOR_F)
    for k, p in d.named_parameters():
        got, want64, want32 = S.sample(p.grad), z['grad64/' + k], z['grad32/' + k]
        err, bound = S.rel_dist(got, want64), _bound(want32, want64, FLOOR_W)
        print(f'{name} grad {k}: error {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append((k, err, bound))
    for k, b in d.named_buffers():
        err, bound = S.rel_dist(b.cpu(), z['buf64/' + k]), _bound(z['buf32/' + k], z['buf64/' + k], FLOOR_F)
        if not err <= bound:
            bad.append((k, err, bound))
    u_after = d.sn_bufs.clone()
    d.eval()
    with torch.no_grad():
        check('eval_out', d(x.detach()).cpu(), FLOOR_F)
    assert torch.equal(d.sn_bufs[:d.engine.layers[0].s_off], u_after[:d.engine.layers[0].s_off])      # eval mode: no iteration
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- C. the trainer
def _sn_b():
    return np.load(os.path.join(GOLDEN, 'sn_b.npz'))


def _fixture_nets(dropout=False):
    """sn_b's networks: a_lrelu_tversky's generator and the spectrally normalised discriminator the fixture stores."""
    import patchgan_amd as pg
    z = _sn_b()
    gold = Golden('a_lrelu_tversky')
    g = pg.UNet(3, 1, 4, use_dropout=dropout, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 8, n_layers=3, spectral_norm=True)
    g.load_state_dict(gold.weights('g0'))
    d.load_state_dict({k: torch.from_numpy(z['d0/' + k].copy()) for k in z['d0/keys']})
    return g.cuda(), d.cuda(), gold.inputs()


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


def _rows(t, x, y, n, train=True):
    return np.array([[float(l[k]) for k in LOSS_KEYS] for l in (t.batch(x, y, train=train) for _ in range(n))])


def test_step_against_the_reference_with_one_iteration_per_step(tmp_path):
    z = _sn_b()
    g, d, (x, y) = _fixture_nets()
    t = _trainer(g, d, tmp_path)
    got = _rows(t, x, y, 4)
    t.flush()
    d.eval()
    got_eval = _rows(t, x, y, 1, train=False)
    bad = []
    for what, a, w32, w64 in (('losses', got, z['losses'], z['losses64']), ('eval', got_eval, z['eval_losses'][None], z['eval_losses64'][None])):
        for j, key in enumerate(LOSS_KEYS):
            err, bound = S.rel_dist(a[:, j], w64[:, j]), _bound(w32[:, j], w64[:, j], FLOOR_F)
            print(f'sn_b {what} {key}: error {err:.3e} bound {bound:.3e}')
            if not err <= bound:
                bad.append((what, key, err, bound))
    assert not bad, bad
    t.release()


STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3)
_MODE_RUNS = {}


def _mode_run(tmp_path_factory, mode):
    if mode not in _MODE_RUNS:
        g, d, (x, y) = _fixture_nets()
        t = _trainer(g, d, tmp_path_factory.mktemp('sn_mode'), mode)
        rows, modes = [], []
        for s in range(STEPS):
            l = t.batch(x, y, train=True)
            rows.append([float(l[k]) for k in LOSS_KEYS])
            modes.append(t.launch_mode)
        t.flush()
        torch.cuda.synchronize()
        _MODE_RUNS[mode] = dict(losses=np.array(rows), modes=modes, d=d.flat.cpu().numpy().copy(), sn=d.sn_bufs.cpu().numpy().copy(),
                                g=g.flat.cpu().numpy().copy())
        t.release()
    return _MODE_RUNS[mode]


@pytest.mark.parametrize('mode', ['eager2', 'graph'])
def test_launch_modes_are_bit_identical(tmp_path_factory, mode):
    one, other = _mode_run(tmp_path_factory, 'eager1'), _mode_run(tmp_path_factory, mode)
    assert other['modes'][3:] == [mode] * (STEPS - 3) and one['modes'] == ['eager1'] * STEPS, (one['modes'], other['modes'])
    assert np.array_equal(one['losses'], other['losses']), one['losses'] - other['losses']
    for k in ('d', 'sn', 'g'):          # D.flat, u / v / sigma, G.flat
        assert np.array_equal(one[k], other[k]), k
    assert np.isfinite(one['losses']).all()


@pytest.mark.parametrize('kind', ['instance', 'instance_affine', 'batch'])
def test_every_norm_layer_with_dropout_ema_and_an_evaluation_step(tmp_path, kind):
    import patchgan_amd as pg
    nl = {'instance': nn.InstanceNorm2d, 'instance_affine': functools.partial(nn.InstanceNorm2d, affine=True), 'batch': nn.BatchNorm2d}[kind]
    torch.manual_seed(3)
    g = pg.UNet(3, 1, 4, use_dropout=True, activation='leakyrelu', final_act='sigmoid').cuda()
    d = pg.Discriminator(4, 8, n_layers=3, norm=True, norm_layer=nl, spectral_norm=True).cuda()
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, ema_decay=0.99, two_streams=True)
    w0 = d.flat.clone()
    rows = _rows(t, x, y, 2)
    t.flush()
    sn_train = d.sn_bufs.clone()
    d.eval()
    g.eval()
    rows_eval = _rows(t, x, y, 1, train=False)
    torch.cuda.synchronize()
    assert np.isfinite(rows).all() and np.isfinite(rows_eval).all()
    assert not torch.equal(d.flat, w0)
    n_uv = d.engine.layers[0].s_off
    assert torch.equal(d.sn_bufs[:n_uv], sn_train[:n_uv])          # an evaluation step with D in eval mode does not iterate
    for k, b in d.named_buffers():
        if k.endswith(('weight_u', 'weight_v')):
            assert abs(float(b.double().norm()) - 1.0) < 1e-6, k
    assert t.ema_generator is not None
    t.release()


def test_bf16_run_stays_finite_and_iterates_in_fp32(tmp_path):
    """Under set_precision('bf16') the normalised weights are fp32 master data like W: u, v of the third step are the float64
    iteration on the fp32 weights that step read, to one rounding."""
    import patchgan_amd as pg
    torch.manual_seed(99)
    g = pg.UNet(3, 1, 16, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda().set_precision('bf16')
    d = pg.Discriminator(4, 32, n_layers=3, spectral_norm=True).cuda().set_precision('bf16')
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path)
    rows = _rows(t, x, y, 2)
    before = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}          # (flushes the second step's Adam(D))
    rows = np.concatenate([rows, _rows(t, x, y, 1)])
    after = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    assert np.isfinite(rows).all() and all(torch.isfinite(v).all() for v in after.values())
    for k in before:
        if k.endswith('weight_orig'):
            stem = k[:-len('_orig')]
            got = dict(u=after[stem + '_u'], v=after[stem + '_v'])
            W, u0, v0 = before[k], before[stem + '_u'], before[stem + '_v']
            t64 = W.double().reshape(W.shape[0], -1).t() @ u0.double()
            ref_v = t64 / t64.norm().clamp_min(S.EPS)
            s64 = W.double().reshape(W.shape[0], -1) @ got['v'].double()
            ref_u = s64 / s64.norm().clamp_min(S.EPS)
            assert S.ratio(got['v'], ref_v, 4 * S.EPS32 * ref_v.abs()) <= 1.0, k
            assert S.ratio(got['u'], ref_u, 4 * S.EPS32 * ref_u.abs()) <= 1.0, k
    t.release()


def test_clipping_takes_the_norm_of_the_mapped_gradient(tmp_path):
    """clip_grad_norm = inf: the reported D norm is the 2-norm of the gradient w.r.t. the STORED weights -- computed here in float64
    from the unmapped gradient of a twin run (the same step with the map switched off), u, v, sigma and the normalised weights."""
    g, d, (x, y) = _fixture_nets()
    t = _trainer(g, d, tmp_path / 'a', clip_grad_norm=float('inf'))
    t.batch(x, y, train=True)
    norm = t.read_grad_stats()['disc']['norm']
    mapped = d.grad_flat.cpu().double()
    eff, sn = d.sn_eff.cpu(), d.sn_bufs.cpu()
    t.release()
    g2, d2, _ = _fixture_nets()
    d2.spectral_grad_map = lambda gflat, *a: gflat
    t2 = _trainer(g2, d2, tmp_path / 'b', clip_grad_norm=float('inf'))
    t2.batch(x, y, train=True)
    t2.flush()
    raw = d2.grad_flat.cpu().double()
    assert torch.equal(d2.sn_bufs.cpu(), sn)          # the twin normalised the same weights
    t2.release()
    want = raw.clone()
    for l in d.engine.layers:
        m = 16 * l.a * l.b
        blk = slice(l.p_off, l.p_off + m)
        u, v, sigma = sn[l.u_off:l.u_off + l.a], sn[l.v_off:l.v_off + 16 * l.b], sn[l.s_off]
        dW = S.grad_map(S.unpack(raw[blk], l.a, l.b), S.unpack(eff[blk], l.a, l.b), u, v, sigma)[0]
        want[blk] = S.pack(dW)
    ref = float(want.norm())
    print(f'D gradient norm: reported {norm:.8g}, float64 of the mapped gradient {ref:.8g}, of the unmapped {float(raw.norm()):.8g}')
    assert abs(norm - ref) <= 1e-6 * ref
    assert abs(float(raw.norm()) - ref) > 1e-3 * ref          # (the map matters at this size)
    assert S.rel_dist(mapped, want) < 1e-5


def test_checkpoints_carry_u_and_v(tmp_path):
    g, d, (x, y) = _fixture_nets()
    t = _trainer(g, d, tmp_path / 'run')
    _rows(t, x, y, 2)
    t.save(2)
    sd = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    want = _rows(t, x, y, 1, train=False)
    t.release()
    saved = torch.load(tmp_path / 'run' / 'discriminator_ep_002.pth')
    assert type(saved) is dict and list(saved) == list(sd)          # (a plain dict, no _metadata: torch's load hook takes it)
    g2, d2, _ = _fixture_nets()
    with torch.no_grad():
        d2.flat.zero_()
        d2.sn_bufs.zero_()
    t2 = _trainer(g2, d2, tmp_path / 'run')
    t2.load_last_checkpoint()
    assert t2.start == 3
    for k, v in d2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    got = _rows(t2, x, y, 1, train=False)
    assert np.array_equal(got, want), got - want
    t2.release()


# ---------------------------------------------------------------------------------------------- D. data parallelism
def _dp_worker(rank, world, port, q, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    g, d, (x, y) = _fixture_nets()
    t = _trainer(g, d, tempfile.mkdtemp())
    xs, ys = shard_batch(x, y, rank, world)
    curve = _rows(t, xs, ys, nsteps)
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, curve, d.flat.cpu().numpy(), d.sn_bufs.cpu().numpy(), g.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_keep_equal_u_v_sigma_and_follow_the_single_process_curve(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    nsteps = 4
    g, d, (x, y) = _fixture_nets()
    t = _trainer(g, d, tmp_path)
    single = _rows(t, x, y, nsteps)
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
    (_, c0, d0, sn0, g0), (_, c1, d1, sn1, g1) = res
    assert np.array_equal(d0, d1) and np.array_equal(sn0, sn1) and np.array_equal(g0, g1)          # weights, u / v / sigma: the same bits
    assert np.allclose(c0, c1, rtol=1e-6)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('spectral dp2 vs single process: max rel err per step', err.max(axis=1))
    assert err.max() < 1e-4, err          # (the bound of tests/test_dp_gpu.py for the plain network)


# ---------------------------------------------------------------------------------------------- E. patchgan_train
def test_train_cli_with_the_yaml_key_writes_torchs_key_set(tmp_path, monkeypatch):
    import patchgan_amd as pg
    from patchgan_amd.train import patchgan_train
    from tests.test_cli_gpu import PLUGIN
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    cfg = {
        'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 1,
                    'train_data': {'images': '4', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
        'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'use_dropout': True},
                         'discriminator': {'filters': 4, 'n_layers': 3, 'spectral_norm': True}},
        'checkpoint_path': str(tmp_path / 'ckpt'),
        'train_params': {'loss_type': 'tversky', 'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3, 'save_freq': 1},
    }
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    G_ep, D_ep = patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])
    assert len(G_ep) == 1 and np.isfinite(G_ep).all() and np.isfinite(D_ep).all()
    sd = torch.load(tmp_path / 'ckpt' / 'discriminator_ep_001.pth')
    want = pg.Discriminator(4, 4, n_layers=3, spectral_norm=True).state_dict()
    assert list(sd) == list(want) and all(sd[k].shape == want[k].shape and sd[k].dtype == want[k].dtype for k in want)
    assert 'model.0.weight_orig' in sd and 'model.0.weight_u' in sd and 'model.0.weight' not in sd
    assert all(abs(float(v.double().norm()) - 1.0) < 1e-6 for k, v in sd.items() if k.endswith(('_u', '_v')))
