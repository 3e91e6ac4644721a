"""The generator's weight average on the GPU: pg_adam_ema_step / pg_adam_ema_step_dev against pg_adam_step and float64 (A),
containment of the five buffers (B), the training trajectory with and without the average in every launch mode (C), the average
read through ema_generator's in-place views (D), patchgan_train / patchgan_infer (E), two data-parallel ranks (F).  Needs an MI355X."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import yaml

from tests.golden_util import LOSS_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PG_OK, PG_EINVAL = 0, -1


def _c64(decay):
    """1 - decay as the kernel forms it (both in float32), as a Python float."""
    return float(np.float32(1.0) - np.float32(decay))


# ---------------------------------------------------------------------------------------------- A. kernel
@pytest.mark.parametrize('decay', [0.5, 0.999])
@pytest.mark.parametrize('n', [3, 4096, 4099], ids=['tail_only', 'body_only', 'body_and_tail'])
def test_kernel_against_adam_step_and_float64(n, decay):
    """p, m, v: bit-identical to pg_adam_step on copies of the same inputs; the device-scalar form: bit-identical to the eager one on
    all four outputs; the average: per step |e' - e64| <= 2^-21 max(|e|, |p'|) with e64 = e + (p' - e) c in float64 from the kernel's
    own fp32 e, p' and c.  The bound is derived: three fp32 roundings give at most 5 * 2^-24 max(|e|, |p'|), contracted or not."""
    from patchgan_amd import engine as E
    g = torch.Generator().manual_seed(7)
    p0, e0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    plain = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    ema = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), e0.to(DEV)]
    dev = [t.clone() for t in ema]
    c = _c64(decay)
    worst = 0.0
    for t in range(1, 6):
        grad = (torch.randn(n, generator=g) * (10.0 ** (t - 3))).to(DEV)          # the gradient scales of test_adam_matches_torch
        e_before = ema[3].clone()
        E.adam_update(plain[0], grad, plain[1], plain[2], step=t, lr=1e-3)
        E.adam_update(ema[0], grad, ema[1], ema[2], step=t, lr=1e-3, ema=ema[3], ema_decay=decay)
        scal = torch.tensor([float(s) for s in E.adam_scalars(t, 1e-3)], dtype=torch.float32, device=DEV)
        E.adam_update(dev[0], grad, dev[1], dev[2], scalars=scal, ema=dev[3], ema_decay=decay)
        torch.cuda.synchronize()
        for a, b, name in zip(plain, ema, 'pmv'):
            assert torch.equal(a, b), (t, name)
        for a, b, name in zip(ema, dev, 'pmve'):
            assert torch.equal(a, b), (t, name)
        e64 = e_before.double() + (ema[0].double() - e_before.double()) * c
        err = (ema[3].double() - e64).abs()
        bound = 2.0 ** -21 * torch.maximum(e_before.double().abs(), ema[0].double().abs())
        worst = max(worst, (err / bound).max().item())
        assert bool((err <= bound).all()), (t, (err / bound).max().item())
    print(f'n={n} decay={decay}: max |e - e64| / (2^-21 max(|e|, |p|)) = {worst:.3f}')
    assert not torch.equal(ema[3], e0.to(DEV)) and not torch.equal(ema[3], ema[0])


@pytest.mark.parametrize('decay', [1.0, float('nan')], ids=['one', 'nan'])
def test_kernel_refuses_a_bad_decay_and_touches_nothing(decay):
    from patchgan_amd import _lib as L
    lib = L.load()
    n = 4099
    g = torch.Generator().manual_seed(8)
    bufs = [torch.randn(n, generator=g).to(DEV) for _ in range(5)]          # p, g, m, v, ema
    scal = torch.tensor([1e-2, 0.03], dtype=torch.float32, device=DEV)
    before = [b.clone() for b in bufs]
    p, gr, m, v, e = (b.data_ptr() for b in bufs)
    assert lib.pg_adam_ema_step(p, gr, m, v, e, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, decay, None) == PG_EINVAL
    assert lib.pg_adam_ema_step_dev(p, gr, m, v, e, n, 0.9, 0.999, 1e-8, scal.data_ptr(), decay, None) == PG_EINVAL
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- B. containment
@pytest.mark.parametrize('dev_scalars', [False, True], ids=['adam_ema_step', 'adam_ema_step_dev'])
def test_adam_ema_containment(dev_scalars):
    from tests import guard_util as G
    from patchgan_amd import _lib as L
    lib = L.load()
    n = 4099
    gen = torch.Generator(device='cuda').manual_seed(7)
    p0, g0, e0 = (torch.randn(n, device='cuda', generator=gen) for _ in range(3))
    p, g, m, v, e = G.flat_from(p0), G.flat_from(g0), G.flat_from(torch.zeros(n)), G.flat_from(torch.zeros(n)), G.flat_from(e0)
    ins = G.Inputs()
    ins.add(g, 'g')
    bc1, sbc2 = 1.0 - 0.9, math.sqrt(1.0 - 0.999)
    if dev_scalars:
        sc = ins.add(G.flat_from(torch.tensor([1e-3 / bc1, sbc2], dtype=torch.float32)), 'scalars')
        rc = lib.pg_adam_ema_step_dev(p.ptr(), g.ptr(), m.ptr(), v.ptr(), e.ptr(), n, 0.9, 0.999, 1e-8, sc.ptr(), 0.75, None)
    else:
        rc = lib.pg_adam_ema_step(p.ptr(), g.ptr(), m.ptr(), v.ptr(), e.ptr(), n, 1e-3, 0.9, 0.999, 1e-8, bc1, sbc2, 0.75, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    for b, name in ((p, 'p'), (m, 'm'), (v, 'v'), (e, 'ema')):
        G.assert_untouched(b, 'all', 'adam_ema ' + name)
    ins.check('adam_ema')
    # first step of Adam from zero moments: p -= lr * g / (|g| + eps); the average moves a quarter of the way to it
    want = p0.double() - 1e-3 * g0.double() / (g0.double().abs() + 1e-8)
    assert (p.inner(torch.float32).double() - want).abs().max().item() < 1e-6
    want_e = e0.double() + (want - e0.double()) * 0.25
    assert (e.inner(torch.float32).double() - want_e).abs().max().item() < 1e-6


# ---------------------------------------------------------------------------------------------- C. trajectory
STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3)
_RUNS = {}


def _inputs(gen):
    x = torch.rand(2, 3, 256, 256, generator=gen)
    y = (torch.rand(2, 1, 256, 256, generator=gen) > 0.7).float()
    return x, y


def _run(tmp_path_factory, mode, decay, precision='fp32', snapshots=False, change=None, steps=STEPS):
    """`steps` training steps from a fixed start (B = 2, 256 x 256, nf = ndf = 16; 32 for bf16, as tests/test_graph_gpu.py) in launch
    mode 'eager1' | 'eager2' | 'graph'.  change = (step, decay): ema_decay is set to that value before that step.  Cached per
    argument set: the references are computed once.  -> dict(losses, g, d, ema, w0, snaps, modes, trainer state)."""
    key = (mode, decay, precision, snapshots, change, steps)
    if key in _RUNS:
        return _RUNS[key]
    import patchgan_amd as pg
    nf = 32 if precision == 'bf16' else 16
    torch.manual_seed(99)
    g = pg.UNet(3, 1, nf, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
    d = pg.Discriminator(4, nf, n_layers=3).cuda()
    if precision == 'bf16':
        g.set_precision('bf16')
        d.set_precision('bf16')
    t = pg.Trainer(g, d, str(tmp_path_factory.mktemp('ema_run')))
    t.graph = mode == 'graph'
    t.two_streams = True if mode == 'eager2' else None
    t.ema_decay = decay
    t.setup_optimizers(1e-3, 2e-3)
    g.train()
    d.train()
    w0 = g.flat.cpu()
    gen = torch.Generator().manual_seed(5)
    rows, snaps, modes, decays = [], [], [], []
    for s in range(steps):
        x, y = _inputs(gen)
        if change is not None and s == change[0]:
            t.ema_decay = change[1]
        l = t.batch(x, y, train=True)
        rows.append([float(l[k]) for k in LOSS_KEYS])
        modes.append(t.launch_mode)
        decays.append(t.ema_decay)
        if snapshots:
            torch.cuda.synchronize()
            snaps.append(g.flat.cpu())          # (fp32 as stored: the recursion below widens them)
    t.flush()
    torch.cuda.synchronize()
    out = dict(losses=np.array(rows), g=g.flat.cpu().numpy().copy(), d=d.flat.cpu().numpy().copy(),
               ema=None if t._ema is None else t._ema.cpu().numpy().copy(), w0=w0, snaps=snaps, modes=modes, decays=decays,
               has_net=t.ema_generator is not None, captured=t.graph_captured(), ngraphs=len(t._graphs))
    t.release()
    _RUNS[key] = out
    return out


def _recursion(w0, snaps, decays):
    e = w0.double()
    for w, decay in zip(snaps, decays):
        e = e + (w.double() - e) * _c64(decay)
    return e


@pytest.mark.parametrize('mode', ['eager1', 'eager2', 'graph'])
def test_training_is_bit_identical_with_and_without_the_average(tmp_path_factory, mode):
    off = _run(tmp_path_factory, mode, None)
    on = _run(tmp_path_factory, mode, 0.99)
    assert off['ema'] is None and not off['has_net'] and on['ema'] is not None and on['has_net']
    assert on['modes'] == off['modes'] and on['modes'][-1] == mode, (on['modes'], off['modes'])
    if mode == 'graph':
        assert on['captured'] and on['modes'][3:] == ['graph'] * (STEPS - 3)          # replays happened
    assert np.array_equal(off['losses'], on['losses']), off['losses'] - on['losses']
    assert np.array_equal(off['g'], on['g']) and np.array_equal(off['d'], on['d'])


def test_training_is_bit_identical_with_and_without_the_average_bf16(tmp_path_factory):
    off = _run(tmp_path_factory, 'eager1', None, 'bf16')
    on = _run(tmp_path_factory, 'eager1', 0.99, 'bf16')
    assert np.array_equal(off['losses'], on['losses'])
    assert np.array_equal(off['g'], on['g']) and np.array_equal(off['d'], on['d'])
    assert on['ema'] is not None and not np.array_equal(on['ema'], on['g'])


def test_the_average_is_the_same_in_every_launch_mode(tmp_path_factory):
    one, two, graph = (_run(tmp_path_factory, m, 0.99)['ema'] for m in ('eager1', 'eager2', 'graph'))
    assert np.array_equal(one, two) and np.array_equal(one, graph)


@pytest.mark.parametrize('decay', [0.99, 0.5])
def test_the_average_follows_the_float64_recursion(tmp_path_factory, decay):
    """One-stream run with the weights snapshotted after every step: e_k = e_{k-1} + (w_k - e_{k-1}) c in float64 from e_0 = w_0.
    Each kernel step is within 2^-21 max(|e|, |w|) of its own float64 step (test A) and the recursion is a contraction (0 < c <= 1),
    so K steps stay within K 2^-21 max|value|.  Decay 0.5: the average has left both the initial and the live weights (not a no-op)."""
    r = _run(tmp_path_factory, 'eager1', decay, snapshots=True)
    want = _recursion(r['w0'], r['snaps'], r['decays'])
    got = torch.from_numpy(r['ema']).double()
    top = max(want.abs().max().item(), max(w.abs().max().item() for w in r['snaps']), r['w0'].abs().max().item())
    err = (got - want).abs().max().item()
    print(f'decay {decay}: max |ema - float64 recursion| = {err:.3e}, bound {STEPS * 2.0 ** -21 * top:.3e}')
    assert err <= STEPS * 2.0 ** -21 * top
    assert np.array_equal(r['g'], r['snaps'][-1].numpy())
    if decay == 0.5:
        assert not np.array_equal(r['ema'], r['w0'].numpy()) and not np.array_equal(r['ema'], r['g'])
        # ... by about what the recursion says: far more than the bound above
        assert (got - r['w0'].double()).abs().max().item() > 100 * STEPS * 2.0 ** -21 * top
        assert (got - r['snaps'][-1].double()).abs().max().item() > 100 * STEPS * 2.0 ** -21 * top


def test_a_changed_decay_takes_effect_on_the_next_step_of_a_captured_run(tmp_path_factory):
    """The decay is a launch argument of the captured Adam(G): a new value is a new kind of step (three launch-by-launch steps with
    the new value, then its own capture), never a replay of the old one."""
    steps, at = 10, 5
    r = _run(tmp_path_factory, 'graph', 0.99, snapshots=True, change=(at, 0.9), steps=steps)
    assert r['modes'][3:at] == ['graph'] * (at - 3) and r['modes'][at:] == ['eager1'] * 3 + ['graph'] * (steps - at - 3), r['modes']
    assert r['decays'] == [0.99] * at + [0.9] * (steps - at) and r['ngraphs'] == 2
    want = _recursion(r['w0'], r['snaps'], r['decays'])
    stale = _recursion(r['w0'], r['snaps'], [0.99] * steps)
    got = torch.from_numpy(r['ema']).double()
    top = max(want.abs().max().item(), max(w.abs().max().item() for w in r['snaps']))
    bound = steps * 2.0 ** -21 * top
    assert (got - want).abs().max().item() <= bound
    assert (got - stale).abs().max().item() > 10 * bound          # (the check can tell the two apart)
    # the weights themselves: those of a run that never changed the decay
    same = _run(tmp_path_factory, 'graph', 0.99, snapshots=True, steps=steps)
    assert np.array_equal(same['g'], r['g']) and np.array_equal(same['losses'], r['losses'])


# ---------------------------------------------------------------------------------------------- D. in-place views
def test_ema_generator_reads_the_buffer_in_place(tmp_path):
    import patchgan_amd as pg
    from patchgan_amd.infer import predict_image
    torch.manual_seed(21)
    g = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
    d = pg.Discriminator(4, 4, n_layers=3).cuda()
    t = pg.Trainer(g, d, str(tmp_path))
    t.ema_decay = 0.5
    t.setup_optimizers(1e-3, 1e-3)
    g.train()
    d.train()
    gen = torch.Generator().manual_seed(5)
    probe = torch.rand(2, 3, 256, 256, generator=gen).cuda()
    image = torch.rand(3, 384, 384, generator=gen).cuda()

    def fresh():
        f = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda().eval()
        f.load_state_dict(t.ema_generator.state_dict(), strict=True)
        return f

    def check(tag):
        with torch.no_grad():
            live = g(probe).clone()
            got, want = t.ema_generator(probe), fresh()(probe)
            assert torch.equal(got, want), tag
            assert not torch.equal(got, live) or tag == 'start', tag
            m1 = predict_image(t.ema_generator, image, 256, 0.9, 0)
            m2 = predict_image(fresh(), image, 256, 0.9, 0)
            assert m1.shape == (384, 384) and np.array_equal(m1, m2), tag
            assert torch.equal(g(probe), live), tag          # the live generator is unaffected by those calls
        return got.clone()

    outs = [check('start')]
    for s in range(3):
        t.batch(*_inputs(gen), train=True)
        if s >= 1:
            outs.append(check(f'after step {s + 1}'))          # (no stale prepared-weight cache: the output moves with the buffer)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert g.training and not t.ema_generator.training


# ---------------------------------------------------------------------------------------------- E. CLI
def test_train_with_ema_then_infer_from_the_ema_file(tmp_path, monkeypatch):
    from tests.test_cli_gpu import PLUGIN
    from patchgan_amd.train import patchgan_train
    from patchgan_amd.infer import patchgan_infer
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    cfg = {
        'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 1,
                    'train_data': {'images': '6', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
        'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'use_dropout': True},
                         'discriminator': {'filters': 4, 'n_layers': 3}},
        'checkpoint_path': str(tmp_path / 'ckpt'),
        'train_params': {'loss_type': 'tversky', 'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3,
                         'save_freq': 1, 'ema_decay': 0.9},
    }
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    G_ep, D_ep = patchgan_train(['-c', 'cfg.yaml', '-n', '2', '-b', '2', '--dataloader_workers', '0'])
    assert len(G_ep) == 2 and all(np.isfinite(G_ep)) and all(np.isfinite(D_ep))
    files = sorted(os.listdir(tmp_path / 'ckpt'))
    assert files == [f'{net}_ep_{ep:03d}.pth' for net in ('discriminator', 'generator_ema', 'generator') for ep in (1, 2)]
    sd, ema = (torch.load(tmp_path / 'ckpt' / f'{n}_ep_002.pth') for n in ('generator', 'generator_ema'))
    assert list(sd) == list(ema) and all(sd[k].shape == ema[k].shape for k in sd)
    assert any(not torch.equal(sd[k], ema[k]) for k in sd)
    icfg = {'dataset': {'type': 'BlobsInfer', 'dataset_path': '2', 'size': 256},
            'model_params': {'gen_filts': 4, 'disc_filts': 4, 'n_disc_layers': 3, 'activation': 'leakyrelu'},
            'checkpoint_paths': {'generator': str(tmp_path / 'ckpt' / 'generator_ema_ep_002.pth'),
                                 'discriminator': str(tmp_path / 'ckpt' / 'discriminator_ep_002.pth')},
            'infer_params': {'output_path': str(tmp_path / 'pred'), 'threshold': 0.5}}
    (tmp_path / 'icfg.yaml').write_text(yaml.safe_dump(icfg))
    patchgan_infer(['-c', 'icfg.yaml'])
    for i in range(2):
        m = np.load(tmp_path / 'pred' / f'blob_{i:03d}.npy')
        assert m.shape == (256, 256) and set(np.unique(m)) <= {0.0, 1.0}


# ---------------------------------------------------------------------------------------------- F. data parallelism
def _dp_worker(rank, world, port, q, base, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(4)
    import patchgan_amd as pg
    from patchgan_amd.parallel import shard_batch
    from tests.golden_util import Golden
    gold = Golden('a_lrelu_tversky')
    c = gold.cfg
    g = pg.UNet(c['in_nc'], c['out_nc'], c['nf'], activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], c['ndf'], n_layers=c['n_layers'], norm=c['norm'])
    g.load_state_dict(gold.weights('g0'))
    d.load_state_dict(gold.weights('d0'))
    g.cuda()
    d.cuda()
    folder = os.path.join(base, f'rank{rank}')
    t = pg.Trainer(g, d, folder)
    t.loss_type = c['loss_type']
    t.bucket_bytes = 64 << 10
    t.ema_decay = 0.99
    t.setup_optimizers(1e-3, 1e-3)
    g.train()
    d.train()
    w0 = g.flat.cpu().numpy().copy()
    xs, ys = shard_batch(*gold.inputs(), rank, world)
    for s in range(nsteps):
        t.batch(xs, ys, train=True)
    t.save(1)
    torch.cuda.synchronize()
    q.put((rank, t._ema.cpu().numpy(), g.flat.cpu().numpy(), w0, sorted(os.listdir(folder))))
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_average_and_rank_0_saves_it(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, str(tmp_path), 3)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, e0, g0, w0, files0), (_, e1, g1, _, files1) = res
    assert np.array_equal(e0, e1) and np.array_equal(g0, g1)
    assert not np.array_equal(e0, w0) and not np.array_equal(e0, g0)          # it moved, and it is not the live weights
    assert files0 == ['discriminator_ep_001.pth', 'generator_ema_ep_001.pth', 'generator_ep_001.pth'] and files1 == []
