"""The optimizer's options on the device: pg_adamw_step / pg_adamw_step_dev against float64 element by element (tests/optim_util.py), their
bit identities with the entry points without a decay, the Adam entry points at betas other than (0.9, 0.999), PG_EINVAL with canaries,
and Trainer.betas / weight_decay / save_optimizer through whole steps: every launch mode, the default trainer's unchanged key and calls,
and the exact resume from optimizer_ep_*.pth.  Needs an MI355X."""
import math
import os

import numpy as np
import pytest
import torch

from tests import optim_util as U
from tests.golden_util import LOSS_KEYS, Golden
from tests.gradclip_util import STAT, scaled

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, INF = float('nan'), float('inf')


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _ok(rc, what):
    assert rc == 0, f'{what} returned {rc}'


def _dev_state(state):
    return [x.float().to(DEV).contiguous() for x in state]


def _stat(coef=1.0, apply=1):
    rec = np.zeros(1, dtype=STAT)
    rec['coef'], rec['apply'], rec['norm'] = coef, apply, 1.0
    return torch.from_numpy(rec.view(np.float64).copy()).to(DEV)


def _adamw(lib, state, t, lr, b1, b2, dm, form='arg', ema=None, ema_decay=0.0, stat=None):
    """One step of pg_adamw_step ('arg') / pg_adamw_step_dev ('dev') on device copies of `state`: (p', m', v', ema') on the device."""
    p, g, m, v = _dev_state(state)
    e = ema.float().to(DEV).contiguous() if ema is not None else None
    n = p.numel()
    bc1, sbc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    eptr, sptr = (e.data_ptr() if e is not None else None), (stat.data_ptr() if stat is not None else None)
    if form == 'arg':
        rc = lib.pg_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), eptr, n, lr, b1, b2, U.ADAM_EPS, bc1, sbc2, dm, ema_decay,
                               sptr, None)
    else:
        sc = torch.tensor(U.scalars(t, lr, b1, b2)[3:] + (dm,), dtype=torch.float32, device=DEV)
        rc = lib.pg_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), eptr, n, b1, b2, U.ADAM_EPS, sc.data_ptr(), ema_decay,
                                   sptr, None)
    _ok(rc, f'pg_adamw_step[{form}]')
    torch.cuda.synchronize()
    return p, m, v, e


def _adam(lib, state, t, lr, b1, b2, form='plain', ema=None, ema_decay=0.0, stat=None, dev=False):
    """The entry points without a decay: 'plain' pg_adam_step, 'ema' pg_adam_ema_step, 'clip' pg_adam_clip_step (ema optional)."""
    p, g, m, v = _dev_state(state)
    e = ema.float().to(DEV).contiguous() if ema is not None else None
    n = p.numel()
    bc1, sbc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    sc = torch.tensor(U.scalars(t, lr, b1, b2)[3:], dtype=torch.float32, device=DEV)
    eptr = e.data_ptr() if e is not None else None
    if form == 'plain':
        rc = (lib.pg_adam_step_dev(*ptrs, n, b1, b2, U.ADAM_EPS, sc.data_ptr(), None) if dev else
              lib.pg_adam_step(*ptrs, n, lr, b1, b2, U.ADAM_EPS, bc1, sbc2, None))
    elif form == 'ema':
        rc = (lib.pg_adam_ema_step_dev(*ptrs, eptr, n, b1, b2, U.ADAM_EPS, sc.data_ptr(), ema_decay, None) if dev else
              lib.pg_adam_ema_step(*ptrs, eptr, n, lr, b1, b2, U.ADAM_EPS, bc1, sbc2, ema_decay, None))
    else:
        rc = (lib.pg_adam_clip_step_dev(*ptrs, eptr, n, b1, b2, U.ADAM_EPS, sc.data_ptr(), ema_decay, stat.data_ptr(), None) if dev else
              lib.pg_adam_clip_step(*ptrs, eptr, n, lr, b1, b2, U.ADAM_EPS, bc1, sbc2, ema_decay, stat.data_ptr(), None))
    _ok(rc, f'pg_adam[{form}]')
    torch.cuda.synchronize()
    return p, m, v, e


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(x, y):
    return all((a is None and b is None) or _bits(a, b) for a, b in zip(x, y))


def _cpu(out):
    return tuple(x.cpu() for x in out[:3])


# ---------------------------------------------------------------------------------------------- 1. the kernel against float64
def _check(lib, case):
    state, sc, dm = U.case_state(case)
    got = _adamw(lib, state, case.t, case.lr, case.b1, case.b2, dm, 'arg')
    other = _adamw(lib, state, case.t, case.lr, case.b1, case.b2, dm, 'dev')
    assert _same(got, other), f'pg_adamw_step_dev differs from pg_adamw_step: {case}'
    return U.adamw_ratios(_cpu(got), state, sc, dm)


@pytest.mark.parametrize('n', U.ADAM_NS, ids=[f'adamw-n{n}' for n in U.ADAM_NS])
def test_adamw_step_against_float64(n):
    lib = _lib()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for case in U.opt_cases(n):
        for k, r in _check(lib, case).items():
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (case, k, r)
    print(f'adamw n={n}: worst ratios {worst}')


def test_adamw_step_multitrip():
    """n = 8388608 + 1027: a second grid trip with a ragged body and a 3-element tail."""
    r = _check(_lib(), U.OPT_BIG)
    print(f'adamw multitrip n={U.OPT_BIG.n}: {r}')
    assert all(v <= 1.0 for v in r.values()), r


# ---------------------------------------------------------------------------------------------- 2. bit identities
@pytest.mark.parametrize('n', (5, 1023, 4099))
def test_bit_identities(n):
    lib = _lib()
    t, lr, b1, b2, decay = 2, 0.1, 0.5, 0.999, 0.99
    case = U.OptCase(n, t, lr, 0.5, b1, b2, True)
    state, sc, dm = U.case_state(case)
    gen = torch.Generator().manual_seed(n)
    ema = torch.randn(n, generator=gen).double()
    coef = 0.37
    stat = _stat(coef, 1)
    # decay_mul == 1: the four (ema, stat) combinations are the entry points without a decay, argument and device forms
    for dev in (False, True):
        form = 'dev' if dev else 'arg'
        assert _same(_adamw(lib, state, t, lr, b1, b2, 1.0, form), _adam(lib, state, t, lr, b1, b2, 'plain', dev=dev))
        assert _same(_adamw(lib, state, t, lr, b1, b2, 1.0, form, ema, decay), _adam(lib, state, t, lr, b1, b2, 'ema', ema, decay, dev=dev))
        assert _same(_adamw(lib, state, t, lr, b1, b2, 1.0, form, stat=stat), _adam(lib, state, t, lr, b1, b2, 'clip', stat=stat, dev=dev))
        assert _same(_adamw(lib, state, t, lr, b1, b2, 1.0, form, ema, decay, stat),
                     _adam(lib, state, t, lr, b1, b2, 'clip', ema, decay, stat, dev=dev))
    # (the clipped form really clipped: its first moment differs from the unclipped one's)
    assert not _bits(_adamw(lib, state, t, lr, b1, b2, 1.0, stat=stat)[1], _adamw(lib, state, t, lr, b1, b2, 1.0)[1])
    # the average: what pg_adam_ema_step gives when fed the decayed p0 = fl32(p * dm); likewise with clipping
    p, g, m, v = state
    p0 = (p.float() * torch.tensor(dm, dtype=torch.float32)).double()
    assert not torch.equal(p0, p)
    assert _same(_adamw(lib, state, t, lr, b1, b2, dm, 'arg', ema, decay), _adam(lib, (p0, g, m, v), t, lr, b1, b2, 'ema', ema, decay))
    assert _same(_adamw(lib, state, t, lr, b1, b2, dm, 'dev', ema, decay, stat), _adam(lib, (p0, g, m, v), t, lr, b1, b2, 'clip', ema, decay, stat))
    # g * coef inside the pass == the pass on fl32(g * coef)
    assert _same(_adamw(lib, state, t, lr, b1, b2, dm, stat=stat)[:3], _adamw(lib, (p, scaled(g, coef), m, v), t, lr, b1, b2, dm)[:3])
    # apply == 0, set by hand: every buffer keeps its bits (the decay included)
    skip = _stat(0.0, 0)
    before = tuple(_dev_state((p, m, v, ema)))
    for form in ('arg', 'dev'):
        assert _same(_adamw(lib, state, t, lr, b1, b2, dm, form, ema, decay, skip), before)
        assert _same(_adamw(lib, state, t, lr, b1, b2, dm, form, stat=skip)[:3], before[:3])
    # m and v do not depend on decay_mul
    a, b = _adamw(lib, state, t, lr, b1, b2, dm), _adamw(lib, state, t, lr, b1, b2, 1.0)
    assert _bits(a[1], b[1]) and _bits(a[2], b[2]) and not _bits(a[0], b[0])


# ---------------------------------------------------------------------------------------------- 3. the existing kernels at the new betas
@pytest.mark.parametrize('b1,b2', U.NEW_BETAS)
@pytest.mark.parametrize('n', U.NEW_BETA_NS)
def test_existing_adam_entry_points_at_other_betas(n, b1, b2):
    lib = _lib()
    stat = _stat(1.0, 1)
    gen = torch.Generator().manual_seed(n)
    ema = torch.randn(n, generator=gen).double()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in U.STEPS:
        for lr in (1e-3, 2e-4):
            for carried in (False, True):
                case = U.OptCase(n, t, lr, None, b1, b2, carried)
                state, sc, _ = U.case_state(case)
                for form, kw in (('plain', {}), ('ema', dict(ema=ema, ema_decay=0.99)), ('clip', dict(stat=stat))):
                    for dev in (False, True):
                        got = _adam(lib, state, t, lr, b1, b2, form, dev=dev, **kw)
                        for k, r in U.adamw_ratios(_cpu(got), state, sc, None).items():
                            worst[k] = max(worst[k], r)
                            assert r <= 1.0, (case, form, dev, k, r)
    print(f'adam at betas ({b1}, {b2}) n={n}: worst ratios {worst}')


# ---------------------------------------------------------------------------------------------- 4. PG_EINVAL, canaries unchanged
def test_einval_touches_nothing():
    lib = _lib()
    n = 1023
    state, _, _ = U.case_state(U.OptCase(n, 2, 0.1, 0.5, 0.9, 0.999, True))
    p, g, m, v = _dev_state(state)
    e = torch.full((n,), 7.0, device=DEV)
    sc = torch.tensor([0.5, 0.04, 0.95], dtype=torch.float32, device=DEV)
    stat = _stat(0.5, 1)
    bufs = (p, g, m, v, e, sc, stat)
    before = [b.clone() for b in bufs]
    P, G, M, V, Em, S, St = (b.data_ptr() for b in bufs)

    def arg(p=P, g=G, m=M, v=V, ema=Em, n=n, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, bc1=0.19, sbc2=0.04, dm=0.95, ed=0.99, stat=St):
        return lib.pg_adamw_step(p, g, m, v, ema, n, lr, b1, b2, eps, bc1, sbc2, dm, ed, stat, None)

    def dev(p=P, g=G, m=M, v=V, ema=Em, n=n, b1=0.9, b2=0.999, eps=1e-8, sc=S, ed=0.99, stat=St):
        return lib.pg_adamw_step_dev(p, g, m, v, ema, n, b1, b2, eps, sc, ed, stat, None)
    for f in (arg, dev):
        for k, ptr in (('p', P), ('g', G), ('m', M), ('v', V)):
            assert f(**{k: None}) == -1 and f(**{k: ptr + 4}) == -1, k
        assert f(ema=Em + 4) == -1 and f(stat=St + 8) == -1 and f(n=0) == -1 and f(n=-1) == -1
        for bad in (NAN, -0.1, 1.0, 2.0, INF):
            assert f(b1=bad) == -1 and f(b2=bad) == -1 and f(b1=bad, ema=None, stat=None) == -1, bad
        for bad in (NAN, -0.1, 1.0, INF):
            assert f(ed=bad) == -1 and f(ed=bad, stat=None) == -1, bad
    for bad in (NAN, 0.0, -0.5, 1.0000001, 2.0, INF, -INF):
        assert arg(dm=bad) == -1 and arg(dm=bad, ema=None) == -1 and arg(dm=bad, stat=None) == -1 and arg(dm=bad, ema=None, stat=None) == -1, bad
    for bad in (0.0, -1.0, NAN):
        assert arg(bc1=bad) == -1 and arg(sbc2=bad) == -1
    assert dev(sc=None) == -1
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # (and the same arguments un-spoilt are accepted; ema_decay is not read without an ema)
    assert arg() == 0 and dev() == 0 and arg(ema=None, ed=NAN) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. Trainer: every step is the float64 AdamW step
GOLD = 'a_lrelu_tversky'
BETAS = ((0.5, 0.999), (0.0, 0.9))


def _nets(seed=99, use_dropout=False, spectral=False, nf=None):
    import patchgan_amd as pg
    c = Golden(GOLD).cfg
    torch.manual_seed(seed)
    g = pg.UNet(c['in_nc'], c['out_nc'], nf or c['nf'], use_dropout=use_dropout, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], nf or c['ndf'], n_layers=c['n_layers'], norm=c['norm'], spectral_norm=spectral)
    g.cuda(), d.cuda()
    g.train(), d.train()
    return g, d


def _batches(steps, seed=5):
    c = Golden(GOLD).cfg
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        x = torch.rand(c['B'], c['in_nc'], c['size'], c['size'], generator=gen)
        out.append((x, (torch.rand(c['B'], c['out_nc'], c['size'], c['size'], generator=gen) > 0.7).float()))
    return out


@pytest.mark.parametrize('combined', [False, True], ids=['plain', 'clip+ema+spectral'])
def test_trainer_steps_are_the_float64_adamw_step(tmp_path, combined):
    import patchgan_amd as pg
    g, d = _nets(spectral=combined)
    t = pg.Trainer(g, d, str(tmp_path))
    t.betas, t.weight_decay = BETAS, (1e-2, None)
    if combined:
        t.clip_grad_norm, t.ema_decay = (1.0, 1.0), 0.99
    lrs = (1e-3, 2e-3)
    t.setup_optimizers(*lrs)
    nets = (('gen', g, 0, 1e-2), ('disc', d, 2, None))
    for step, (x, y) in enumerate(_batches(2), 1):
        t.flush()
        torch.cuda.synchronize()
        before = {name: [b.detach().double().cpu() for b in (net.flat, t._adam[i], t._adam[i + 1])] for name, net, i, _ in nets}
        ema0 = t._ema.double().cpu() if combined else None
        t.batch(x, y, train=True)
        t.flush()
        torch.cuda.synchronize()
        stats = t.read_grad_stats() if combined else None
        for (name, net, i, wd), lr, (b1, b2) in zip(nets, lrs, BETAS):
            p, m, v = before[name]
            grad = net.grad_flat.double().cpu()
            if combined:
                assert stats[name]['skipped'] == 0 and 0.0 < stats[name]['coef'] <= 1.0
                grad = scaled(grad, stats[name]['coef'])
            got = tuple(b.detach().cpu() for b in (net.flat, t._adam[i], t._adam[i + 1]))
            dm = U.decay_mul(lr, wd) if wd is not None else None
            r = U.adamw_ratios(got, (p, grad, m, v), U.scalars(step, lr, b1, b2), dm)
            print(f'step {step} {name}: {r}')
            assert all(val <= 1.0 for val in r.values()), (step, name, r)
            assert bool(grad.abs().sum() > 0) and not torch.equal(got[0].double(), p)
            if dm is not None:          # (the decay is visible: the step without it misses the bound)
                assert U.adamw_ratios(got, (p, grad, m, v), U.scalars(step, lr, b1, b2), None)['p'] > 1.0
        if combined:
            c = float(np.float32(1.0) - np.float32(0.99))
            assert U.ema_ratio(t._ema.cpu(), ema0, g.flat.detach().cpu(), c) <= 1.0
    assert (t._t_g, t._t_d) == (2, 2)


# ---------------------------------------------------------------------------------------------- 6. launch modes
def _run(tmp_path, tag, steps=5, graph=False, two_streams=None, optim=True, lr_change_at=4):
    import patchgan_amd as pg
    g, d = _nets(nf=16)
    t = pg.Trainer(g, d, str(tmp_path / tag))
    t.graph, t.two_streams = graph, two_streams
    if optim:
        t.betas, t.weight_decay = BETAS, (1e-2, 5e-3)
    t.setup_optimizers(1e-3, 2e-3)
    rows, used = [], []
    for s, (x, y) in enumerate(_batches(steps)):
        if s == lr_change_at:
            t.gen_lr, t.dsc_lr = 5e-4, 1e-4          # the third scalar of a replayed step follows the learning rate
        l = t.batch(x, y, train=True)
        rows.append([float(l[k]) for k in LOSS_KEYS])
        used.append(t.launch_mode)
    t.flush()
    torch.cuda.synchronize()
    return np.array(rows), [b.cpu().numpy().copy() for b in (g.flat, d.flat) + tuple(t._adam)], used, t


def test_launch_modes_give_the_same_bits(tmp_path):
    one = _run(tmp_path, 'one')
    assert set(one[2]) == {'eager1'}
    two = _run(tmp_path, 'two', two_streams=True)
    assert set(two[2]) == {'eager2'}
    rep = _run(tmp_path, 'graph', graph=True)
    assert rep[2] == ['eager1'] * 3 + ['graph'] * 2, rep[2]
    st = next(iter(rep[3]._graphs.values()))
    assert st.scal.numel() == 6 and st.host[0].numel() == 6
    for other in (two, rep):
        assert np.array_equal(one[0], other[0])
        assert all(np.array_equal(a, b) for a, b in zip(one[1], other[1]))
        assert (other[3]._t_g, other[3]._t_d) == (5, 5)
    # (the settings took effect: a default trainer ends elsewhere)
    plain = _run(tmp_path, 'plain', optim=False)
    assert not np.array_equal(one[1][0], plain[1][0]) and not np.array_equal(one[1][1], plain[1][1])


def test_default_trainer_keeps_its_kind_key_and_calls(tmp_path, monkeypatch):
    """With the settings at their defaults the step's kind key is the one without the feature and the library calls are those of
    before: two pg_adam_step per training step, pg_adam_step_dev under capture, never pg_adamw_*."""
    import patchgan_amd as pg
    from patchgan_amd import _lib as L, engine as E
    real = L.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith('pg_adam'):
                calls.append(name)
            return getattr(real, name)
    g, d = _nets(nf=16)
    t = pg.Trainer(g, d, str(tmp_path))
    t.graph = True
    t.setup_optimizers(1e-3, 2e-3)
    (x, y), = _batches(1)
    monkeypatch.setattr(E.L, 'load', lambda: Spy())
    for _ in range(5):
        t.batch(x, y, train=True)
    t.flush()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls == ['pg_adam_step'] * 6 + ['pg_adam_step_dev'] * 2, calls          # three eager steps and the capture; replays launch nothing by name
    c = Golden(GOLD).cfg
    dims = (c['B'], c['size'], c['size'], c['in_nc'], c['out_nc'])
    xd, yd = x.cuda(), y.cuda()
    key = t._kind_key(xd, yd, False, dims, True)
    assert key == t._kind_key_base(xd, yd, False, dims, True) and t._optim_key() == ()
    assert next(iter(t._graphs.values())).scal.numel() == 4
    t.betas = (0.9, 0.999)          # set, even to the default values: another kind of step
    assert t._kind_key(xd, yd, False, dims, True) == key + (('optim', ((0.9, 0.999), (0.9, 0.999)), (None, None)),)
    assert t._kind_key(xd, yd, False, dims, False) == t._kind_key_base(xd, yd, False, dims, False)


# ---------------------------------------------------------------------------------------------- 7. exact resume
def _resume_trainer(folder, save_optimizer):
    import patchgan_amd as pg
    g, d = _nets(seed=42, use_dropout=True)
    t = pg.Trainer(g, d, folder)
    t.diffaug = 'translation,cutout'
    t.betas, t.weight_decay, t.save_optimizer = BETAS, (1e-2, 5e-3), save_optimizer
    return t


def _final(t, losses):
    t.flush()
    torch.cuda.synchronize()
    return dict(weights=[b.cpu().numpy().copy() for b in (t.generator.flat, t.discriminator.flat)],
                moments=[b.cpu().numpy().copy() for b in t._adam], steps=(t._t_g, t._t_d, t._step), aug=t.read_diffaug_params(),
                losses=[[float(l[k]) for k in LOSS_KEYS] for l in losses])


def _run_b(folder, save_optimizer, data):
    t = _resume_trainer(folder, save_optimizer)
    t.setup_optimizers(1e-3, 2e-3)
    for x, y in data[:2]:
        t.batch(x, y, train=True)
    t.save(1)
    files = sorted(os.listdir(folder))
    t = _resume_trainer(folder, save_optimizer)          # fresh networks, a fresh trainer
    t.load_last_checkpoint()
    assert t.start == 2
    t.setup_optimizers(1e-3, 2e-3)          # as train() does
    return _final(t, [t.batch(x, y, train=True) for x, y in data[2:]]), files


def test_exact_resume(tmp_path):
    data = _batches(4)
    ta = _resume_trainer(str(tmp_path / 'a'), None)
    ta.setup_optimizers(1e-3, 2e-3)
    a = _final(ta, [ta.batch(x, y, train=True) for x, y in data][2:])
    b, files = _run_b(str(tmp_path / 'b'), True, data)
    assert files == ['discriminator_ep_001.pth', 'generator_ep_001.pth', 'optimizer_ep_001.pth']
    assert a['steps'] == b['steps'] == (4, 4, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a['weights'], b['weights']))
    assert all(np.array_equal(x, y) for x, y in zip(a['moments'], b['moments']))
    assert np.array_equal(a['aug'], b['aug']) and a['losses'] == b['losses']
    sd = torch.load(str(tmp_path / 'b' / 'optimizer_ep_001.pth'))
    assert sd['trainer']['step'] == 2 and sd['trainer']['diffaug_counter'] == 2 and (sd['trainer']['t_g'], sd['trainer']['t_d']) == (2, 2)
    # the control: the same run without the optimizer file restarts Adam, dropout and the augmentation stream -- and differs
    c, files = _run_b(str(tmp_path / 'c'), None, data)
    assert files == ['discriminator_ep_001.pth', 'generator_ep_001.pth']          # exactly the files of before
    assert c['steps'] == (2, 2, 2)
    assert not np.array_equal(a['weights'][0], c['weights'][0]) and not np.array_equal(a['moments'][0], c['moments'][0])
    assert a['losses'] != c['losses']
