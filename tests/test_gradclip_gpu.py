"""Gradient-norm clipping on the GPU: pg_grad_norm and pg_adam_clip_step / pg_adam_clip_step_dev against float64 per element (A),
non-finite gradients (B), the accumulators (C), containment (D), refusals (E); the trainer: monitor mode against off, clipping in every
launch mode, the teacher-forced float64 check, a poisoned batch, two data-parallel ranks, patchgan_train (F).  The references,
tolerances and cases are tests/gradclip_util.py's (held to torch's clip_grad_norm_ + Adam in tests/test_gradclip_cpu.py).
Needs an MI355X."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests import gradclip_util as U
from tests.golden_util import LOSS_KEYS
from tests.lossopt_util import ADAM_EPS, B1, B2

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PG_OK, PG_EINVAL = 0, -1
INF = float('inf')
DECAY = 0.999
EMA_C = float(np.float32(1.0) - np.float32(DECAY))


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _report(name, r):
    print(f'{name}: ' + '  '.join(f'{k} {v:.3f}' for k, v in sorted(r.items())))


def _ema_of(state):
    return state[0] * 0.5 + 0.25


def _record(stat):
    return stat.cpu().numpy().view(U.STAT)[0]


def _call(lib, state, sc, mx, form, ema=None, stat=None):
    """pg_grad_norm, then pg_adam_clip_step ('arg') or pg_adam_clip_step_dev ('dev') on copies of the state -> everything on the host."""
    p, g, m, v = (x.float().to(DEV) for x in state)
    e = ema.float().to(DEV) if ema is not None else None
    n = g.numel()
    stat = torch.zeros(8, dtype=torch.float64, device=DEV) if stat is None else stat
    assert lib.pg_grad_norm_workspace_bytes(n) == 8 * U.norm_blocks(n)
    ws = torch.full((U.norm_blocks(n),), float('nan'), dtype=torch.float64, device=DEV)          # (every partial must be written)
    assert all(x.data_ptr() % 16 == 0 for x in (p, g, m, v, stat))
    assert lib.pg_grad_norm(g.data_ptr(), n, mx, ws.data_ptr(), ws.numel() * 8, stat.data_ptr(), None) == PG_OK
    t, lr = U.T_LR
    eptr = e.data_ptr() if e is not None else None
    if form == 'arg':
        rc = lib.pg_adam_clip_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), eptr, n, lr, B1, B2, ADAM_EPS, 1.0 - B1 ** t,
                                   math.sqrt(1.0 - B2 ** t), DECAY, stat.data_ptr(), None)
    else:
        scal = torch.tensor(sc[3:], dtype=torch.float32, device=DEV)
        rc = lib.pg_adam_clip_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), eptr, n, B1, B2, ADAM_EPS, scal.data_ptr(),
                                       DECAY, stat.data_ptr(), None)
    assert rc == PG_OK
    torch.cuda.synchronize()
    r = _record(stat)
    assert torch.equal(g.cpu().view(torch.int32), state[1].float().view(torch.int32)), 'g was rewritten'
    return dict(sumsq=float(r['sumsq']), norm=float(r['norm']), coef=float(r['coef']), apply=int(r['apply']), rec=r.tobytes(),
                p=p.cpu(), m=m.cpu(), v=v.cpu(), ema=e.cpu() if e is not None else None, steps=int(r['steps']),
                clipped=int(r['clipped']), skipped=int(r['skipped']))


def _plain(lib, state, ema=None):
    """pg_adam_step / pg_adam_ema_step on copies of the same state."""
    p, g, m, v = (x.float().to(DEV) for x in state)
    n = g.numel()
    t, lr = U.T_LR
    tail = (lr, B1, B2, ADAM_EPS, 1.0 - B1 ** t, math.sqrt(1.0 - B2 ** t))
    if ema is None:
        rc = lib.pg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *tail, None)
        e = None
    else:
        e = ema.float().to(DEV)
        rc = lib.pg_adam_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, *tail, DECAY, None)
    assert rc == PG_OK
    torch.cuda.synchronize()
    return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), ema=e.cpu() if e is not None else None)


def _same(a, b, keys):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys if a[k] is not None)


def _check_case(lib, case, worst):
    """All four forms of one case: float64 ratios of the plain and the EMA call, the device-scalar forms bit-identical to them, a
    repeated call bit-identical including the status block, coef == 1 bit-identical to the unclipped kernels."""
    state, sc, mx = U.case_state(case)
    ema = _ema_of(state)
    got = _call(lib, state, sc, mx, 'arg')
    got_e = _call(lib, state, sc, mx, 'arg', ema)
    for k, x in U.clip_ratios(got, state, sc, mx).items():
        worst[k] = max(worst.get(k, 0.0), x)
    for k, x in U.clip_ratios(got_e, state, sc, mx, ema, EMA_C).items():
        worst[k] = max(worst.get(k, 0.0), x)
    assert got['rec'] == got_e['rec'] and _same(got, got_e, 'pmv'), (case, 'the average changes p, m or v')
    for e, ref in ((None, got), (ema, got_e)):
        dev = _call(lib, state, sc, mx, 'dev', e)
        assert dev['rec'] == ref['rec'] and _same(dev, ref, ('p', 'm', 'v', 'ema')), (case, 'dev differs from arg')
    again = _call(lib, state, sc, mx, 'arg', ema)
    assert again['rec'] == got_e['rec'] and _same(again, got_e, ('p', 'm', 'v', 'ema')), (case, 'a repeated call differs')
    clips = case.clip == 'below' and U.norm_ref(state[1]) > 0.0
    assert (got['coef'] < 1.0) == clips and (got['steps'], got['clipped'], got['skipped']) == (1, int(clips), 0), case
    if not clips:
        assert got['coef'] == 1.0, case
        assert _same(got, _plain(lib, state), 'pmv'), (case, 'coef == 1 differs from pg_adam_step')
        assert _same(got_e, _plain(lib, state, ema), ('p', 'm', 'v', 'ema')), (case, 'coef == 1 differs from pg_adam_ema_step')
    else:
        assert not _same(got, _plain(lib, state), 'pmv') or case.n == 1, (case, 'clipping changed nothing')


# ---------------------------------------------------------------------------------------------- A. kernels against float64
@pytest.mark.parametrize('n', U.NORM_NS, ids=lambda n: f'n{n}')
def test_norm_and_clipped_adam_against_float64(n):
    lib = _lib()
    worst = {}
    cases = [c for c in U.clip_cases() if c.n == n]
    assert cases
    for case in cases:
        _check_case(lib, case, worst)
    _report(f'clip n={n} ({len(cases)} cases)', worst)
    assert max(worst.values()) <= 1.0, worst


def test_norm_and_clipped_adam_multitrip():
    """n = 8 388 608 + 1027: five trips of the norm's grid, a second trip of Adam's, a ragged body and 3 tail elements."""
    lib, worst = _lib(), {}
    assert U.BIG_CASE.n > 4 * U.TRIP and U.BIG_CASE.n % 4 == 3
    _check_case(lib, U.BIG_CASE, worst)
    _report(f'clip multitrip n={U.BIG_CASE.n}', worst)
    assert max(worst.values()) <= 1.0, worst


def test_huge_gradients_keep_a_finite_norm():
    """All |g| >= 1e20: the fp32 sum of squares is inf (tests/test_gradclip_cpu.py), the norm is 1e20 sqrt(n) or more and stored."""
    lib = _lib()
    state, sc, mx = U.case_state(U.ClipCase(4099, 'huge', 'below'))
    got = _call(lib, state, sc, mx, 'arg')
    assert math.isfinite(got['norm']) and got['norm'] >= 1e20 * math.sqrt(4099) and got['apply'] == 1 and 0.0 < got['coef'] < 1e-20
    r = U.clip_ratios(got, state, sc, mx)
    assert max(r.values()) <= 1.0, r


# ---------------------------------------------------------------------------------------------- B. non-finite gradients
@pytest.mark.parametrize('poison', U.POISONS, ids=lambda p: f'{p[0]}-{p[1]}')
def test_a_non_finite_gradient_skips_the_step(poison):
    lib = _lib()
    state, sc, mx = U.case_state((U.ClipCase(U.POISON_N, 'unit', 'below'),) + poison)
    ema = _ema_of(state)
    for form in ('arg', 'dev'):
        for e in (None, ema):
            got = _call(lib, state, sc, mx, form, e)
            assert U.clip_ratios(got, state, sc, mx, e, EMA_C) == {'skip': 0.0}, (form, e is not None)
            assert (got['steps'], got['clipped'], got['skipped']) == (1, 0, 1) and not math.isfinite(got['norm'])
    clean = U.clip_inputs(U.POISON_N, 'unit')          # (the same state without the planted value does update)
    assert _call(lib, clean, sc, mx, 'arg')['apply'] == 1


# ---------------------------------------------------------------------------------------------- C. accumulators
def test_accumulators_over_a_clipped_an_unclipped_and_a_skipped_call():
    lib = _lib()
    stat = torch.zeros(8, dtype=torch.float64, device=DEV)
    n = 4099
    a, sc, _ = U.case_state(U.ClipCase(n, 'unit', 'below'))
    b = U.clip_inputs(n, 'small')
    c = U.poisoned(a, 'tail', float('nan'))
    na, nb = U.norm_ref(a[1]), U.norm_ref(b[1])
    r1 = _call(lib, a, sc, na / 4, 'arg', stat=stat)
    r2 = _call(lib, b, sc, nb * 4, 'dev', stat=stat)
    r3 = _call(lib, c, sc, 1.0, 'arg', stat=stat)
    assert (r1['steps'], r1['clipped'], r1['skipped']) == (1, 1, 0) and (r2['steps'], r2['clipped'], r2['skipped']) == (2, 1, 0)
    assert (r3['steps'], r3['clipped'], r3['skipped']) == (3, 1, 1) and r3['coef'] == 0.0 and r3['apply'] == 0
    rec = _record(stat)
    tol = n * U.ACC + 2.0 ** -52
    assert abs(float(rec['max_norm']) - max(na, nb)) <= tol * max(na, nb)
    assert abs(float(rec['sum_norm']) - (na + nb)) <= 2 * tol * (na + nb)
    assert na > nb          # (the maximum is the FIRST call's: it is kept, not overwritten by the last finite norm)


# ---------------------------------------------------------------------------------------------- D. containment
@pytest.mark.parametrize('n', [4099, U.TRIP + U.CHUNK + 3], ids=['one_trip', 'two_trips'])
def test_grad_norm_containment(n):
    from tests import guard_util as G
    lib = _lib()
    _, g0, _, _ = U.clip_inputs(n, 'unit')
    g = G.flat_from(g0.float())
    ws, stat = G.flat(8 * U.norm_blocks(n)), G.flat_from(torch.zeros(8, dtype=torch.float64))
    ins = G.Inputs()
    ins.add(g, 'g')
    rc = lib.pg_grad_norm(g.ptr(), n, 1.0, ws.ptr(), ws.nbytes, stat.ptr(), None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    G.assert_untouched(ws, 'all', 'grad_norm workspace')
    G.assert_untouched(stat, 'all', 'grad_norm status block')
    ins.check('grad_norm')
    rec = stat.inner(torch.float64).cpu().numpy().view(U.STAT)[0]
    assert abs(float(rec['sumsq']) - U.sumsq_ref(g0)) <= n * U.ACC * U.sumsq_ref(g0) and int(rec['steps']) == 1
    assert not bool(torch.isnan(ws.inner(torch.float64)).any())          # every partial of the declared size was written


@pytest.mark.parametrize('skip', [False, True], ids=['apply', 'skip'])
@pytest.mark.parametrize('with_ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('dev_scalars', [False, True], ids=['adam_clip_step', 'adam_clip_step_dev'])
def test_adam_clip_containment(dev_scalars, with_ema, skip):
    from tests import guard_util as G
    lib = _lib()
    n = 4099
    gen = torch.Generator(device='cuda').manual_seed(7)
    p0, g0, e0 = (torch.randn(n, device='cuda', generator=gen) for _ in range(3))
    p, g, m, v = G.flat_from(p0), G.flat_from(g0), G.flat_from(torch.zeros(n)), G.flat_from(torch.zeros(n))
    e = G.flat_from(e0) if with_ema else None
    rec = np.zeros(1, dtype=U.STAT)
    rec[0] = (2.0, 0.0 if skip else 0.5, 0 if skip else 1, 0, 1, 1, 0, 2.0, 2.0, 4.0)
    ins = G.Inputs()
    ins.add(g, 'g')
    stat = ins.add(G.flat_from(torch.from_numpy(rec.view(np.float64).copy())), 'status block')
    if skip:
        for b, name in ((p, 'p'), (m, 'm'), (v, 'v'), (e, 'ema')):
            ins.add(b, name)
    bc1, sbc2 = 1.0 - 0.9, math.sqrt(1.0 - 0.999)
    eptr = e.ptr() if with_ema else None
    if dev_scalars:
        sc = ins.add(G.flat_from(torch.tensor([1e-3 / bc1, sbc2], dtype=torch.float32)), 'scalars')
        rc = lib.pg_adam_clip_step_dev(p.ptr(), g.ptr(), m.ptr(), v.ptr(), eptr, n, 0.9, 0.999, 1e-8, sc.ptr(), 0.75, stat.ptr(), None)
    else:
        rc = lib.pg_adam_clip_step(p.ptr(), g.ptr(), m.ptr(), v.ptr(), eptr, n, 1e-3, 0.9, 0.999, 1e-8, bc1, sbc2, 0.75, stat.ptr(), None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    for b, name in ((p, 'p'), (m, 'm'), (v, 'v')) + (((e, 'ema'),) if with_ema else ()):
        G.assert_untouched(b, 'all', 'adam_clip ' + name)
    ins.check('adam_clip')
    if not skip:
        # first step of Adam from zero moments: p -= lr * g' / (|g'| + eps) with g' = g / 2; the average moves a quarter of the way
        gh = g0.double() * 0.5
        want = p0.double() - 1e-3 * gh / (gh.abs() + 1e-8)
        assert (p.inner(torch.float32).double() - want).abs().max().item() < 1e-6
        assert (m.inner(torch.float32).double() - 0.1 * gh).abs().max().item() < 1e-6
        if with_ema:
            assert (e.inner(torch.float32).double() - (e0.double() + (want - e0.double()) * 0.25)).abs().max().item() < 1e-6


# ---------------------------------------------------------------------------------------------- E. refusals
def test_refusals_touch_nothing():
    lib = _lib()
    n = 4099
    gen = torch.Generator().manual_seed(8)
    bufs = [torch.randn(n + 4, generator=gen).to(DEV) for _ in range(5)]          # p, g, m, v, ema
    stat = torch.full((10,), 3.0, dtype=torch.float64, device=DEV)
    ws = torch.full((U.norm_blocks(n) + 1,), 5.0, dtype=torch.float64, device=DEV)
    scal = torch.tensor([1e-2, 0.03], dtype=torch.float32, device=DEV)
    before = [b.clone() for b in bufs + [stat, ws, scal]]
    p, g, m, v, e = (b.data_ptr() for b in bufs)
    s, w, wb = stat.data_ptr(), ws.data_ptr(), 8 * U.norm_blocks(n)
    for mx in (0.0, -1.0, float('nan'), -INF):
        assert lib.pg_grad_norm(g, n, mx, w, wb, s, None) == PG_EINVAL, mx
    for args in ((None, n, 1.0, w, wb, s), (g, n, 1.0, None, wb, s), (g, n, 1.0, w, wb, None), (g, 0, 1.0, w, wb, s),
                 (g + 4, n, 1.0, w, wb, s), (g, n, 1.0, w + 4, wb, s), (g, n, 1.0, w, wb, s + 8), (g, n, 1.0, w, wb - 8, s),
                 (g, n, 1.0, w, 0, s)):
        assert lib.pg_grad_norm(*args, None) == PG_EINVAL, args
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03)
    for ptrs in ((None, g, m, v, e), (p, None, m, v, e), (p, g, None, v, e), (p, g, m, None, e), (p + 4, g, m, v, e), (p, g + 4, m, v, None),
                 (p, g, m, v, e + 4)):
        assert lib.pg_adam_clip_step(*ptrs, n, *tail, 0.9, s, None) == PG_EINVAL, ptrs
        assert lib.pg_adam_clip_step_dev(*ptrs, n, 0.9, 0.999, 1e-8, scal.data_ptr(), 0.9, s, None) == PG_EINVAL, ptrs
    for st in (None, s + 8):
        assert lib.pg_adam_clip_step(p, g, m, v, e, n, *tail, 0.9, st, None) == PG_EINVAL
        assert lib.pg_adam_clip_step_dev(p, g, m, v, None, n, 0.9, 0.999, 1e-8, scal.data_ptr(), 0.9, st, None) == PG_EINVAL
    assert lib.pg_adam_clip_step_dev(p, g, m, v, e, n, 0.9, 0.999, 1e-8, None, 0.9, s, None) == PG_EINVAL
    for decay in (1.0, float('nan')):
        assert lib.pg_adam_clip_step(p, g, m, v, e, n, *tail, decay, s, None) == PG_EINVAL
        assert lib.pg_adam_clip_step_dev(p, g, m, v, e, n, 0.9, 0.999, 1e-8, scal.data_ptr(), decay, s, None) == PG_EINVAL
    torch.cuda.synchronize()
    for a, b in zip(bufs + [stat, ws, scal], before):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- F. the trainer
STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3)
MODES = ('eager1', 'eager2', 'graph')
_RUNS = {}


def _inputs(gen):
    x = torch.rand(2, 3, 256, 256, generator=gen)
    y = (torch.rand(2, 1, 256, 256, generator=gen) > 0.7).float()
    return x, y


def _nets(kind):
    """'instance': the shapes of tests/test_ema_gpu.py (nf = ndf = 16, InstanceNorm, dropout off); 'dnorm': a norm=True discriminator;
    'batchnorm': nn.BatchNorm2d in both networks."""
    import patchgan_amd as pg
    torch.manual_seed(99)
    nl = nn.BatchNorm2d if kind == 'batchnorm' else nn.InstanceNorm2d
    g = pg.UNet(3, 1, 16, norm_layer=nl, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
    d = pg.Discriminator(4, 16, n_layers=3, norm=kind != 'instance', norm_layer=nl).cuda()
    return g, d


def _trainer(tmp_path_factory, mode, clip, decay=None, kind='instance'):
    import patchgan_amd as pg
    g, d = _nets(kind)
    t = pg.Trainer(g, d, str(tmp_path_factory.mktemp('clip_run')))
    t.graph = mode == 'graph'
    t.two_streams = True if mode == 'eager2' else None
    t.ema_decay = decay
    t.clip_grad_norm = clip
    t.setup_optimizers(1e-3, 2e-3)
    g.train()
    d.train()
    return t


def _run(tmp_path_factory, mode, clip, decay=None, probe=False, kind='instance'):
    """STEPS training steps from a fixed start in one launch mode; probe: read_grad_stats() after every step (the norms per step).
    Cached per argument set."""
    key = (mode, clip, decay, probe, kind)
    if key in _RUNS:
        return _RUNS[key]
    t = _trainer(tmp_path_factory, mode, clip, decay, kind)
    g, d = t.generator, t.discriminator
    gen = torch.Generator().manual_seed(5)
    rows, modes, norms = [], [], []
    for s in range(STEPS):
        l = t.batch(*_inputs(gen), train=True)
        rows.append([float(l[k]) for k in LOSS_KEYS])
        modes.append(t.launch_mode)
        if probe:
            st = t.read_grad_stats()
            norms.append((st['gen']['norm'], st['disc']['norm']))
    t.flush()
    torch.cuda.synchronize()
    out = dict(losses=np.array(rows), g=g.flat.cpu().numpy().copy(), d=d.flat.cpu().numpy().copy(), modes=modes, norms=norms,
               ema=None if t._ema is None else t._ema.cpu().numpy().copy(), captured=t.graph_captured(),
               stats=t.read_grad_stats() if clip is not None else None,
               rec=t._clip[0].cpu().numpy().tobytes() if clip is not None else None, has_clip=t._clip is not None)
    t.release()
    _RUNS[key] = out
    return out


def _clip_values(tmp_path_factory, kind='instance'):
    """(gen, disc) max-norms: 0.25 x the smallest norm a monitor run of the same steps reported, per network."""
    r = _run(tmp_path_factory, 'eager1', INF, probe=True, kind=kind)
    assert len(r['norms']) == STEPS and all(math.isfinite(a) and a > 0 and math.isfinite(b) and b > 0 for a, b in r['norms'])
    return 0.25 * min(a for a, _ in r['norms']), 0.25 * min(b for _, b in r['norms'])


@pytest.mark.parametrize('decay', [None, 0.99], ids=['plain', 'ema'])
@pytest.mark.parametrize('mode', MODES)
def test_monitor_mode_is_bit_identical_to_off(tmp_path_factory, mode, decay):
    off = _run(tmp_path_factory, mode, None, decay)
    on = _run(tmp_path_factory, mode, INF, decay)
    assert not off['has_clip'] and on['has_clip']
    assert on['modes'] == off['modes'] and on['modes'][-1] == mode, (on['modes'], off['modes'])
    if mode == 'graph':
        assert on['captured'] and on['modes'][3:] == ['graph'] * (STEPS - 3)          # replays happened
    assert np.array_equal(off['losses'], on['losses']), off['losses'] - on['losses']
    assert np.array_equal(off['g'], on['g']) and np.array_equal(off['d'], on['d'])
    if decay is not None:
        assert np.array_equal(off['ema'], on['ema'])
    for net in ('gen', 'disc'):
        s = on['stats'][net]
        assert (s['steps'], s['clipped'], s['skipped'], s['coef']) == (STEPS, 0, 0, 1.0), s
        assert all(math.isfinite(s[k]) and s[k] > 0 for k in ('norm', 'max_norm', 'mean_norm')) and s['mean_norm'] <= s['max_norm'], s


def test_reading_the_norm_every_step_changes_nothing(tmp_path_factory):
    a, b = _run(tmp_path_factory, 'eager1', INF), _run(tmp_path_factory, 'eager1', INF, probe=True)
    assert np.array_equal(a['g'], b['g']) and np.array_equal(a['d'], b['d']) and a['rec'] == b['rec']
    assert b['stats']['gen']['max_norm'] == pytest.approx(max(n for n, _ in b['norms']), rel=2.0 ** -23)


def test_clipping_clips_and_every_launch_mode_agrees(tmp_path_factory):
    clip = _clip_values(tmp_path_factory)
    runs = {m: _run(tmp_path_factory, m, clip, 0.99) for m in MODES}
    for m, r in runs.items():
        assert r['modes'][-1] == m, r['modes']
        for net in ('gen', 'disc'):
            s = r['stats'][net]
            assert s['steps'] == STEPS and s['clipped'] == s['steps'] and s['skipped'] == 0 and 0.0 < s['coef'] < 1.0, (m, net, s)
    assert runs['graph']['captured'] and runs['graph']['modes'][3:] == ['graph'] * (STEPS - 3)
    one = runs['eager1']
    for m in ('eager2', 'graph'):
        r = runs[m]
        assert np.array_equal(one['g'], r['g']) and np.array_equal(one['d'], r['d']) and np.array_equal(one['ema'], r['ema']), m
        assert one['rec'] == r['rec'], m
        assert np.array_equal(one['losses'], r['losses']), m
    off = _run(tmp_path_factory, 'eager1', None, 0.99)
    assert not np.array_equal(off['g'], one['g']) and not np.array_equal(off['d'], one['d'])          # it did change the trajectory


def test_a_changed_max_norm_takes_effect_on_the_next_step_of_a_captured_run(tmp_path_factory):
    """The max-norms are launch arguments of the captured pg_grad_norm: a new value is a new kind of step (three launch-by-launch
    steps, then its own capture), never a replay of the old one.  Every step's coefficient is the one of the value set at that step."""
    a = _clip_values(tmp_path_factory)
    b = (a[0] / 2, a[1] / 4)
    steps, at = 10, 5
    t = _trainer(tmp_path_factory, 'graph', a)
    gen = torch.Generator().manual_seed(5)
    modes = []
    for s in range(steps):
        if s == at:
            t.clip_grad_norm = b
        t.batch(*_inputs(gen), train=True)
        modes.append(t.launch_mode)
        st = t.read_grad_stats()
        for net, mx in zip(('gen', 'disc'), a if s < at else b):
            want = U.coef_ref(st[net]['norm'], mx)
            assert want < 1.0 and abs(st[net]['coef'] - want) <= (U.EPS32 + 2.0 ** -40) * want, (s, net, st[net], mx)
    assert modes[3:at] == ['graph'] * (at - 3) and modes[at:] == ['eager1'] * 3 + ['graph'] * (steps - at - 3), modes
    assert len(t._graphs) == 2
    t.release()


@pytest.mark.parametrize('kind', ['instance', 'dnorm', 'batchnorm'])
@pytest.mark.parametrize('mode', ['eager1', 'graph'])
def test_teacher_forced_steps_against_float64(tmp_path_factory, mode, kind):
    """Every step on its own: from the state before and the flat gradient the step left behind, the float64 norm over the PARAMETERS'
    gradients (the packed layout's padding floats must not contribute), the coefficient from the norm read back, and Adam on
    fl32(g * coef) with the trainer's own step count."""
    clip = _clip_values(tmp_path_factory, kind)
    t = _trainer(tmp_path_factory, mode, clip, None, kind)
    gen = torch.Generator().manual_seed(5)
    worst, modes = {}, []
    nets = (('g', t.generator, 0, 1e-3, clip[0]), ('d', t.discriminator, 2, 2e-3, clip[1]))
    for s in range(STEPS):
        t.flush()
        torch.cuda.synchronize()
        before = {w: (net.flat.cpu().double(), t._adam[k].cpu().double(), t._adam[k + 1].cpu().double()) for w, net, k, _, _ in nets}
        t.batch(*_inputs(gen), train=True)
        t.flush()
        torch.cuda.synchronize()
        modes.append(t.launch_mode)
        rec = t._clip[0].cpu().numpy().view(U.STAT)
        for i, (w, net, k, lr, mx) in enumerate(nets):
            p0, m0, v0 = before[w]
            gflat = net.grad_flat.cpu().double()
            grads = [q.grad.detach().cpu().double().reshape(-1) for q in net.parameters()]
            assert sum(x.numel() for x in grads) <= gflat.numel()
            r = rec[i]
            got = dict(sumsq=float(r['sumsq']), norm=float(r['norm']), coef=float(r['coef']), apply=int(r['apply']),
                       p=net.flat.cpu(), m=t._adam[k].cpu(), v=t._adam[k + 1].cpu())
            step = t._t_g if w == 'g' else t._t_d
            assert step == s + 1 and int(r['steps']) == s + 1 and int(r['clipped']) == s + 1
            for key, x in U.clip_ratios(got, (p0, gflat, m0, v0), U.adam_scalars(step, lr), mx, norm_of=grads).items():
                worst[f'{w}.{key}'] = max(worst.get(f'{w}.{key}', 0.0), x)
    t.release()
    _report(f'teacher-forced {mode} {kind}', worst)
    assert modes[-1] == mode and (mode != 'graph' or modes[3:] == ['graph'] * (STEPS - 3)), modes
    assert max(worst.values()) <= 1.0, worst


def _poisoned_run(tmp_path_factory, clip):
    t = _trainer(tmp_path_factory, 'eager1', clip, 0.99)
    g, d = t.generator, t.discriminator
    gen = torch.Generator().manual_seed(5)

    def state():
        t.flush()
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (g.flat, d.flat, t._ema) + tuple(t._adam)]
    snaps = []
    for s in range(4):
        x, y = _inputs(gen)
        if s == 2:
            x[1, 2, 100, 17] = float('nan')
        t.batch(x, y, train=True)
        snaps.append(state())
    stats = t.read_grad_stats() if clip is not None else None
    t.release()
    return snaps, stats


def test_a_poisoned_batch_is_skipped_and_training_goes_on(tmp_path_factory):
    snaps, stats = _poisoned_run(tmp_path_factory, INF)
    for a, b in zip(snaps[1], snaps[2]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))          # weights, average and moments of both networks keep their bits
    for net in ('gen', 'disc'):
        assert (stats[net]['steps'], stats[net]['skipped'], stats[net]['clipped']) == (4, 1, 0), stats
    for a, b in zip(snaps[2], snaps[3]):          # the following clean step updates normally
        assert not np.array_equal(a, b) and np.isfinite(b).all()
    without, _ = _poisoned_run(tmp_path_factory, None)
    for a, b in zip(without[1], snaps[1]):
        assert np.array_equal(a, b)                                          # the same run up to the poisoned step ...
    assert np.isnan(without[3][0]).any() and np.isnan(without[3][1]).any()  # ... which the feature alone survives


# ---- data parallelism
DP_CFG = dict(out_nc=1, nf=8, final_act='sigmoid', norm=False, loss_type='tversky')


def _dp_trainer(gw, dw, folder, clip):
    import patchgan_amd as pg
    cfg = DP_CFG
    g = pg.UNet(3, cfg['out_nc'], cfg['nf'], activation='leakyrelu', final_act=cfg['final_act'], use_dropout=True)
    d = pg.Discriminator(3 + cfg['out_nc'], cfg['nf'], n_layers=3, norm=cfg['norm'])
    g.load_state_dict(gw)
    d.load_state_dict(dw)
    g.cuda()
    d.cuda()
    g._seed_base = 99
    t = pg.Trainer(g, d, folder)
    t.loss_type = cfg['loss_type']
    t.bucket_bytes = 256 << 10
    t.clip_grad_norm = clip
    t.setup_optimizers(1e-3, 1e-3)
    g.train()
    d.train()
    return t


def _dp_steps(t, x, y, nsteps):
    """-> (loss curve, step 1's (gen, disc) norms, weights, the status blocks' bytes)."""
    curve, first = [], None
    for s in range(nsteps):
        l = t.batch(x, y, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
        if s == 0:
            st = t.read_grad_stats()
            first = (st['gen']['norm'], st['disc']['norm'])
    stats = t.read_grad_stats()
    torch.cuda.synchronize()
    return (np.array(curve), first, t.generator.flat.cpu().numpy(), t.discriminator.flat.cpu().numpy(), t._clip[0].cpu().numpy().tobytes(),
            stats)


def _dp_worker(rank, world, port, q, gw, dw, x, y, nsteps, clip):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    t = _dp_trainer(gw, dw, tempfile.mkdtemp(), clip)
    xs, ys = shard_batch(x, y, rank, world)
    q.put((rank,) + _dp_steps(t, xs, ys, nsteps))
    dist.destroy_process_group()


def test_two_ranks_clip_the_global_gradient_alike(tmp_path):
    import patchgan_amd as pg
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    cfg = DP_CFG
    torch.manual_seed(31)
    g = pg.UNet(3, cfg['out_nc'], cfg['nf'], activation='leakyrelu', final_act=cfg['final_act'], use_dropout=True)
    d = pg.Discriminator(3 + cfg['out_nc'], cfg['nf'], n_layers=3, norm=cfg['norm'])
    gw = {k: v.clone() for k, v in g.state_dict().items()}
    dw = {k: v.clone() for k, v in d.state_dict().items()}
    gen = torch.Generator().manual_seed(32)
    x = torch.rand(4, 3, 256, 256, generator=gen)
    y = (torch.rand(4, cfg['out_nc'], 256, 256, generator=gen) > 0.6).float()
    nsteps = 4
    # the max-norms: a quarter of the smallest norm of a monitor run, as in the single-process tests
    t = _dp_trainer(gw, dw, str(tmp_path / 'monitor'), INF)
    norms = []
    for s in range(nsteps):
        t.batch(x, y, train=True)
        st = t.read_grad_stats()
        norms.append((st['gen']['norm'], st['disc']['norm']))
    t.release()
    clip = (0.25 * min(a for a, _ in norms), 0.25 * min(b for _, b in norms))
    t = _dp_trainer(gw, dw, str(tmp_path / 'single'), clip)
    single, first, _, _, _, sstats = _dp_steps(t, x, y, nsteps)
    t.release()
    assert all(sstats[k]['clipped'] == sstats[k]['steps'] == nsteps for k in ('gen', 'disc')), sstats
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, gw, dw, x, y, nsteps, clip)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, f0, g0, d0, rec0, st0), (_, c1, f1, g1, d1, rec1, st1) = res
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1) and rec0 == rec1 and f0 == f1
    assert np.allclose(c0, c1, rtol=1e-6)
    assert all(st0[k]['clipped'] == st0[k]['steps'] == nsteps and st0[k]['skipped'] == 0 for k in ('gen', 'disc')), st0
    for name, got, want in (('G', f0[0], first[0]), ('D', f0[1], first[1])):
        print(f'dp2 step-1 {name} gradient norm {got:.7g} vs single process {want:.7g}: relative {abs(got - want) / want:.2e}')
        assert abs(got - want) <= 1e-5 * want, (name, got, want)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('dp2 clipped vs single process: max rel err per step', err.max(axis=1))
    assert err.max() < 1e-4, err


# ---- patchgan_train
def test_train_with_clip_grad_norm_prints_and_records_the_norms(tmp_path, monkeypatch, capsys):
    from tests.test_cli_gpu import PLUGIN
    import patchgan_amd.train as T
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    cfg = {
        'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 1,
                    'train_data': {'images': '6', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
        'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'use_dropout': True},
                         'discriminator': {'filters': 4, 'n_layers': 3}},
        'checkpoint_path': str(tmp_path / 'ckpt'),
        'train_params': {'loss_type': 'tversky', 'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3,
                         'save_freq': 1, 'clip_grad_norm': [1e-3, None]},
    }
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    seen = []
    real = T.Trainer

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)
    monkeypatch.setattr(T, 'Trainer', Spy)
    G_ep, D_ep = T.patchgan_train(['-c', 'cfg.yaml', '-n', '2', '-b', '2', '--dataloader_workers', '0'])
    assert len(G_ep) == 2 and all(np.isfinite(G_ep)) and all(np.isfinite(D_ep))
    t = seen[0]
    assert t.clip_grad_norm == (1e-3, None) and [h['epoch'] for h in t.grad_history] == [1, 2]
    for h in t.grad_history:          # three batches of two per epoch; the accumulators restart every epoch
        assert (h['gen']['steps'], h['gen']['clipped'], h['gen']['skipped']) == (3, 3, 0) and h['gen']['max_norm'] > 1e-3, h
        assert h['disc']['steps'] == 0                                         # the discriminator's member is None: plain Adam
    out = capsys.readouterr().out
    assert out.count('Gradient norm -- generator: mean ') == 2 and 'clipped 3/3  skipped 0' in out
