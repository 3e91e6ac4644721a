"""Trainer's opt-in features turned on TOGETHER, on the GPU, against ONE composed float64 oracle (tests/combo_util.ComboOracleTrainer) and
against themselves across the launch modes.  Needs an MI355X.

For every case of combo_util.CASES (pairwise coverage of gan objective x spectral normalisation x differentiable augmentation x
segmentation objective x D norm x accumulation x clipping x optimizer settings x weight average; tests/test_combo_cpu.py holds the list
to its conditions and the oracle to the oracles the suite already trusts):
  A. the first closed update's gradient, parameter by parameter, the clipping coefficients and sigma per layer against float64;
  B. three closed updates as one number against float64 (bound: 3 x the float32 oracle's own distance, combo_util.COMBO_NOISE);
  C. for each modelled interaction error (combo_util.MUTATIONS) the device's result at least 10 x the bound from the mutated oracle;
  D. the four launch modes bit for bit, also on BatchNorm / affine-InstanceNorm / bf16 / dropout variants of the everything-on case;
  E. one scripted run whose settings change under capture, against the same script launch by launch."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from tests import combo_util as C
from tests import spectral_util as S
from tests.golden_util import LOSS_KEYS

pytestmark = pytest.mark.gpu

UPDATES = 6          # per run: Trainer.GRAPH_WARM_STEPS = 3 closed updates launch by launch, then three in the decreed mode
MODES = ('eager1', 'eager2', 'graph', 'graph2')
VARIANTS = {'batchnorm': dict(norm_layer=nn.BatchNorm2d), 'inaffine': dict(norm_layer=functools.partial(nn.InstanceNorm2d, affine=True)),
            'bf16': dict(nf=32, ndf=32), 'dropout': dict(use_dropout=True)}
_RUNS, _ORACLE = {}, {}


def _settings(name, **over):
    s = C.trainer_settings(name)
    if C.CASES[name]['diffaug']:
        s.update(diffaug=C.ALL_POLICY, diffaug_seed=C.CASES[name]['aug_seed'])
    s.update(over)
    return s


def _trainer(g, d, folder, settings, mode=None, lr=(C.LR, C.LR)):
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(folder))
    for k, v in settings.items():
        setattr(t, k, v)
    t.setup_optimizers(*lr)
    if mode is not None:
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    g.train()
    d.train()
    return t


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.uint8).numpy().copy() if t is not None else None


def _buffers(t):
    """Every buffer a training call may write, as bytes: the weights, both networks' Adam moments, the weight average, u / v / sigma,
    the grad-stats blocks, the diffaug counter and (BatchNorm) the modules' other buffers."""
    g, d = t.generator, t.discriminator
    t.flush()
    torch.cuda.synchronize()
    out = {'G.flat': _bits(g.flat), 'D.flat': _bits(d.flat), 'ema': _bits(t._ema), 'sn_bufs': _bits(getattr(d, 'sn_bufs', None)),
           'grad_stats': _bits(t._clip[0]) if t._clip is not None else None, 'diffaug_counter': _bits(t._aug_counter)}
    out.update({f'adam{i}': _bits(m) for i, m in enumerate(t._adam)})
    for tag, net in (('G', g), ('D', d)):
        out.update({f'{tag}.buffer.{k}': _bits(b) for k, b in net.named_buffers()})
    return out


def _first_update(t, case):
    """What the first closed update left: every parameter's gradient, the clipping coefficients, sigma per layer."""
    g, d = t.generator, t.discriminator
    t.flush()
    torch.cuda.synchronize()
    out = {'g_grads': {k: p.grad.detach().cpu().clone() for k, p in g.named_parameters()},
           'd_grads': {k: p.grad.detach().cpu().clone() for k, p in d.named_parameters()}}
    if case['clip'] is not None:
        stats = t.read_grad_stats()
        out['coef_g'], out['coef_d'], out['stats'] = stats['gen']['coef'], stats['disc']['coef'], stats
    if case['spectral']:
        sn = d.sn_bufs.cpu()
        out['sigma'] = [float(sn[l.s_off]) for l in d.engine.layers if l.sn]
    return out


def _state(t):
    g, d = t.generator, t.discriminator
    out = {**{'g.' + k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
           **{'d.' + k: v.detach().cpu().clone() for k, v in d.state_dict().items()}}
    if t.ema_generator is not None:
        out.update({'ema.' + k: v.detach().cpu().clone() for k, v in t.ema_generator.state_dict().items()})
    return out


def _hip_run(factory, name, mode, variant=None):
    """UPDATES closed updates of a case (or of a variant of it) in one launch mode, run once and shared: the losses of every call, the
    launch mode and augmentation table of every call, how often the shared-pass entry point ran per call, the first update's gradients,
    the state after the third update and every buffer's bytes at the end."""
    key = (name, mode, variant)
    if key in _RUNS:
        return _RUNS[key]
    case = C.CASES[name]
    g, d = C.modules(name, **dict(VARIANTS[variant] if variant else {}))
    sd = ({k: v.detach().clone() for k, v in g.state_dict().items()}, {k: v.detach().clone() for k, v in d.state_dict().items()})
    g, d = g.cuda(), d.cuda()
    if variant == 'bf16':
        g.set_precision('bf16')
        d.set_precision('bf16')
        assert g.engine.act_bf and d.engine.act_bf          # bf16 storage really is on at this width
    t = _trainer(g, d, factory.mktemp('combo'), _settings(name), mode, case['lr'])
    parts = []
    forward_part = d.engine.forward_part
    d.engine.forward_part = lambda *a, **kw: (parts.append(1), forward_part(*a, **kw))[1]
    k = case['accumulate'] or 1
    run = dict(sd=sd, losses=[], modes=[], parts=[], first=None, state3=None)
    for call in range(UPDATES * k):
        parts.clear()
        l = t.batch(*C.inputs(name, call), train=True)
        run['losses'].append([float(l[key_]) for key_ in LOSS_KEYS])
        run['modes'].append(t.launch_mode)
        run['parts'].append(len(parts))
        if case['diffaug']:
            # (the device's own table IS the one the oracle is teacher-forced with)
            assert np.array_equal(t.read_diffaug_params(), C.table(name, call)), call
        if call == k - 1:
            run['first'] = _first_update(t, case)
        if call == 3 * k - 1:
            t.flush()
            torch.cuda.synchronize()
            run['state3'] = _state(t)
    run['losses'] = np.array(run['losses'])
    run['buffers'] = _buffers(t)
    run['updates'] = (t._t_g, t._t_d)
    del d.engine.forward_part
    t.release()
    _RUNS[key] = run
    return run


def _oracle_run(factory, name, mutate=None, dtype=torch.float64, updates=3):
    """The case through ComboOracleTrainer on the weights the device run began with (computed once, shared, never modified)."""
    key = (name, mutate, dtype, updates)
    if key not in _ORACLE:
        gsd, dsd = _hip_run(factory, name, 'eager1')['sd']
        _ORACLE[key] = C.run(name, dtype, mutate, updates, gsd, dsd)
    return _ORACLE[key]


def _grad_report(name, got, want):
    """[(parameter, error, bound)] of the first update's gradients against the float64 oracle's."""
    dist = C.grad_dists(got, want)
    return [(p, e, C.grad_bound(C.COMBO_NOISE[name]['grad'][p])) for p, e in dist.items()]


def _curve(name, hip, want):
    calls = want['losses'].shape[0]
    return C.curve_dist(hip['losses'][:calls], hip['state3'], want['losses'], want['state'])


# ---------------------------------------------------------------------------------------------- A. one closed update, per parameter
@pytest.mark.parametrize('name', list(C.CASES))
def test_first_update_against_the_float64_oracle(tmp_path_factory, name):
    """Every parameter's gradient of both networks after the first closed update (with `accumulate` the window's mean), read from .grad
    after flush(): relative L2 from ComboOracleTrainer(float64) < 2e-2 and <= 8 x noise + 1e-3, noise the float32 oracle's own distance
    for that parameter (combo_util.COMBO_NOISE).  The clipping coefficients of read_grad_stats() to 1e-5 relative, sigma per layer within
    tests/test_spectral_gpu.py's bound, and -- the way tests/test_share_dfake_gpu.py tells the two apart -- whether the step took the
    shared D(fake) pass (two half passes per call) as the planner's predicate says.
    Measured on an MI355X (the parameter with the largest error / bound; error, bound, ratio): everything 2.7e-06 1.0e-03 0.003, plain
    4.4e-06 1.6e-03 0.003, hinge_shared 3.5e-06 1.1e-03 0.003, hinge_sn_ref 5.2e-04 5.1e-03 0.101 (d.model.0.bias, a near-cancelling
    sum), lsgan_sn 4.5e-06 1.0e-03 0.004, lsgan_ce 4.2e-06 1.0e-03 0.004, lsgan_ref 8.7e-06 1.1e-03 0.008, vanilla_sn 7.4e-06 1.1e-03
    0.007, vanilla_ce 2.6e-06 1.0e-03 0.003, vanilla_accum 7.3e-06 1.0e-03 0.007; coefficients to 1.2e-07, sigma to 1.0e-07."""
    case = C.CASES[name]
    hip, want = _hip_run(tmp_path_factory, name, 'eager1'), _oracle_run(tmp_path_factory, name)
    assert hip['modes'] == ['eager1'] * len(hip['modes'])
    rows = _grad_report(name, hip['first'], want['first'])
    for p, e, bound in rows:
        print(f'{name} {p:44s} error {e:.2e} bound {bound:.2e} ratio {e / bound:.3f}')
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f'{name}: gradients, worst parameter {worst[0]} error {worst[1]:.3e} bound {worst[2]:.3e} ratio {worst[1] / worst[2]:.3f}')
    assert all(e < 2e-2 and e <= bound for _p, e, bound in rows), worst
    if case['clip'] is not None:
        for net in ('g', 'd'):
            got_c, want_c = hip['first']['coef_' + net], want['first']['coef_' + net]
            print(f'{name}: clipping coefficient {net} {got_c:.8e} oracle {want_c:.8e}')
            assert abs(got_c - want_c) <= 1e-5 * want_c, (net, got_c, want_c)
        assert min(hip['first']['coef_g'], hip['first']['coef_d']) < 0.9
    if case['spectral']:
        from tests.test_spectral_gpu import FLOOR_F, _bound
        s32 = _oracle_run(tmp_path_factory, name, None, torch.float32, 1)['first']['sigma']
        s64 = want['first']['sigma']
        assert len(hip['first']['sigma']) == len(s64)
        for got_s, (stem, w64) in zip(hip['first']['sigma'], s64.items()):
            err, bound = S.rel_dist([got_s], [w64]), _bound([s32[stem]], [w64], FLOOR_F)
            print(f'{name}: sigma {stem} {got_s:.8f} oracle {w64:.8f} error {err:.2e} bound {bound:.2e}')
            assert err <= bound, (stem, err, bound)
    shared = 2 if C.SHARED[name] else 0
    assert hip['parts'] == [shared] * len(hip['parts']), (hip['parts'], C.SHARED[name])


# ---------------------------------------------------------------------------------------------- B. three closed updates, one number
@pytest.mark.parametrize('name', list(C.CASES))
def test_three_updates_against_the_float64_oracle(tmp_path_factory, name):
    """3, 6 or 9 calls: the largest relative error among every loss scalar of every call (floor 1e-6) and, after the third update, every
    parameter tensor of both networks, the weight average and u / v (relative max-norm), against ComboOracleTrainer(float64); the bound
    is 3 x COMBO_NOISE[case]['curve'], the float32 oracle's own distance.
    Measured on an MI355X (distance, bound, ratio; the largest term is a weight tensor every time but in `everything`, whose clipped steps keep the weights
    within 2.8e-07; the losses alone are at 8e-08 .. 1e-04): everything 1.56e-06 8.71e-06 0.179, plain 2.10e-03 4.22e-03 0.497, hinge_shared 2.69e-04 8.61e-02 0.003, hinge_sn_ref
    2.04e-04 9.46e-04 0.215, lsgan_sn 4.71e-04 4.89e-03 0.096, lsgan_ce 2.15e-03 1.29e-01 0.017, lsgan_ref 2.37e-04 1.72e-03 0.138,
    vanilla_sn 1.26e-03 8.94e-03 0.140, vanilla_ce 3.82e-03 1.33e-01 0.029, vanilla_accum 5.38e-04 1.82e-03 0.295."""
    hip, want = _hip_run(tmp_path_factory, name, 'eager1'), _oracle_run(tmp_path_factory, name)
    e_l, e_w = _curve(name, hip, want)
    bound = 3 * C.COMBO_NOISE[name]['curve']
    print(f'{name} three updates vs float64 oracle: losses {e_l:.3e}, state {e_w:.3e}; distance {max(e_l, e_w):.3e}, bound {bound:.3e}, '
          f'ratio {max(e_l, e_w) / bound:.3f}')
    assert max(e_l, e_w) <= bound, (e_l, e_w, bound)
    k = C.CASES[name]['accumulate'] or 1
    assert hip['updates'] == (UPDATES, UPDATES) and len(hip['losses']) == UPDATES * k


# ---------------------------------------------------------------------------------------------- C. sensitivity on the device
@pytest.mark.parametrize('mutation', [m for m in C.MUTATIONS if C.SEPARATES[m] is not None])
def test_the_device_result_is_far_from_the_mutated_oracle(tmp_path_factory, mutation):
    """For the case that separates a mutation (combo_util.SEPARATES), the device's run lies at least 10 x the bound from the MUTATED
    float64 oracle, in the gradients or in the curve, and within the bound of the true one.  No launch of its own: the runs above.
    Measured on an MI355X, in units of 10 x the bound: fake_other_row 26.8, no_adjoint 61.6, sigma_before_iteration 984, iterate_per_pass
    49.9, map_once_at_close 3.8, clip_per_call 1.8e13 (the mutated oracle's closed gradient has norm 1e-8), decay_every_call 17.4,
    ema_every_call 10.4, mean_twice 97.8, weights_skip_dice 86.6, real_label_on_gen 10.5, stale_dfake 5.8."""
    name = C.SEPARATES[mutation]
    hip, true, mutated = _hip_run(tmp_path_factory, name, 'eager1'), _oracle_run(tmp_path_factory, name), _oracle_run(tmp_path_factory, name, mutation)
    calls = true['losses'].shape[0]
    far, far_g, far_c = C.separation(name, hip['first'], hip['losses'][:calls], hip['state3'], mutated, true)
    print(f'{mutation} on {name}: the device lies {far:.2f} x (10 x the bound) from the mutated oracle (gradients {far_g:.2f}, curve {far_c:.2f})')
    assert far >= 1.0, (mutation, name, far_g, far_c)
    assert all(e <= bound for _p, e, bound in _grad_report(name, hip['first'], true['first']))
    assert max(_curve(name, hip, true)) <= 3 * C.COMBO_NOISE[name]['curve']


# ---------------------------------------------------------------------------------------------- D. the launch modes
def _same_bits(one, other, what):
    assert np.array_equal(one['losses'], other['losses']), (what, one['losses'] - other['losses'])
    assert np.isfinite(one['losses']).all()
    assert set(one['buffers']) == set(other['buffers'])
    for k, a in one['buffers'].items():
        b = other['buffers'][k]
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (what, k)
    assert one['updates'] == other['updates']


def _decreed(run, name, mode):
    warm = 3 * (C.CASES[name]['accumulate'] or 1)
    return run['modes'][:warm] == ['eager1'] * warm and run['modes'][warm:] == [mode] * (len(run['modes']) - warm)


@pytest.mark.parametrize('mode', MODES[1:])
@pytest.mark.parametrize('name', list(C.CASES))
def test_launch_modes_are_bit_identical(tmp_path_factory, name, mode):
    """Three warm updates and three in the decreed mode: every loss of every call, G.flat, D.flat, both networks' Adam moments, the
    weight average, sn_bufs, the grad-stats blocks and the diffaug counter carry eager1's bits, and launch_mode shows the mode ran."""
    one, other = _hip_run(tmp_path_factory, name, 'eager1'), _hip_run(tmp_path_factory, name, mode)
    assert _decreed(one, name, 'eager1') and _decreed(other, name, mode), (one['modes'], other['modes'])
    _same_bits(one, other, (name, mode))
    case = C.CASES[name]
    for key, on in (('ema', case['ema']), ('sn_bufs', case['spectral']), ('grad_stats', case['clip'] is not None), ('diffaug_counter', case['diffaug'])):
        assert (one['buffers'][key] is not None) == bool(on), key
    if case['diffaug']:
        assert int(one['buffers']['diffaug_counter'].view(np.int64)[0]) == len(one['modes'])


@pytest.mark.parametrize('variant,mode', [(v, m) for v in ('batchnorm', 'inaffine', 'bf16') for m in MODES[1:]] + [('dropout', 'eager2')])
def test_launch_modes_on_variants_of_the_everything_case(tmp_path_factory, variant, mode):
    """The everything-on case with a BatchNorm discriminator, an affine-InstanceNorm discriminator, on bf16 networks with bf16 storage
    (nf = ndf = 32: the narrowest width that stores bf16) and with generator dropout (not capturable: eager1 against eager2).  No
    oracle: the same-bits claim of Trainer's docstring is the assertion."""
    one, other = _hip_run(tmp_path_factory, C.EVERYTHING, 'eager1', variant), _hip_run(tmp_path_factory, C.EVERYTHING, mode, variant)
    assert _decreed(one, C.EVERYTHING, 'eager1') and _decreed(other, C.EVERYTHING, mode), (one['modes'], other['modes'])
    _same_bits(one, other, (variant, mode))
    assert not np.array_equal(one['buffers']['G.flat'], _bits(C.modules(C.EVERYTHING, **dict(VARIANTS[variant]))[0].flat))


# ---------------------------------------------------------------------------------------------- E. settings changing under capture
SCRIPT_CASE = 'lsgan_sn'          # lsgan on logits with label smoothing, spectral D, diffaug on the shared pass, weighted focal+dice, the average


def _script():
    """[(settings that change, training calls, close a short window after this many calls or None)]; the last entry is the first."""
    base = _settings(SCRIPT_CASE, accumulate=None, betas=(0.9, 0.99), weight_decay=(1e-3, 1e-3), clip_grad_norm=(100.0, 2.0), focal_gamma=2)
    w = list(base['class_weights'])
    # (betas, the decay and the max-norms are SET from the first call on: each change below is a change of value under a key that exists)
    steps = [(dict(base), 3, None), (dict(real_label=1.0), 3, None), (dict(focal_gamma=3), 3, None), (dict(class_weights=w[::-1]), 3, None),
             (dict(betas=C.OPTIM_BETAS), 3, None), (dict(weight_decay=C.OPTIM_DECAY), 3, None), (dict(clip_grad_norm=(50.0, 1.0)), 3, None),
             (dict(ema_decay=0.9), 3, None), (dict(diffaug_seed=77), 3, None), (dict(diffaug='translation,cutout'), 3, None),
             (dict(accumulate=2), 6, None), (dict(accumulate=3), 8, 2), (dict(accumulate=None), 3, None), (dict(base), 3, None)]
    assert w[::-1] != w
    return base, steps


def _scripted(factory, graph):
    from patchgan_amd import engine as E
    base, steps = _script()
    g, d = C.modules(SCRIPT_CASE)
    t = _trainer(g.cuda(), d.cuda(), factory.mktemp('script'), base)
    t.graph, t.GRAPH_WARM_STEPS = graph, 1
    captures = []
    capture = t._capture
    t._capture = lambda *a, **kw: (captures.append(t._step), capture(*a, **kw))[1]
    now, seen, rows, modes, expect, call = {}, {}, [], [], [], 0
    for change, calls, short in steps:
        for k, v in change.items():
            setattr(t, k, v)
        now.update(change)
        acc, done = now.get('accumulate'), 0
        for i in range(calls):
            if short is not None and i == short:
                assert t.step_accumulated() and not t.step_accumulated()
                done = 0
            phase = E.accum_phase(done, acc) if acc else None
            done = 0 if phase in (None, 'close') else done + 1
            kind = (tuple(sorted((k, repr(v)) for k, v in now.items())), phase)
            seen[kind] = seen.get(kind, 0) + 1
            l = t.batch(*C.inputs(SCRIPT_CASE, call % 7), train=True)
            rows.append([float(l[k]) for k in LOSS_KEYS])
            modes.append(t.launch_mode)
            expect.append(seen[kind] > 1)
            call += 1
    out = dict(losses=np.array(rows), modes=modes, expect=expect, buffers=_buffers(t), updates=(t._t_g, t._t_d), captures=captures,
               kinds=len(seen), last_block=call - steps[-1][1])
    t.release()
    return out


def test_settings_changing_under_capture_reach_the_replay(tmp_path_factory):
    """graph = True with one warm step per kind, and real_label, focal_gamma, class_weights, betas, weight_decay, clip_grad_norm,
    ema_decay, diffaug_seed, the diffaug policy and accumulate (None -> 2 -> 3, a short window closed by step_accumulated(), -> None)
    changed one after another, then back to the first settings -- against the identical script launch by launch.  Every loss and every
    final buffer is equal bit for bit; the first call of each new kind is not a replay and the later ones are; the first kind, evicted
    long since (MAX_GRAPHS), is captured again on return and still agrees.  A setting missing from the kind key would replay the old
    value here."""
    eager, replay = _scripted(tmp_path_factory, False), _scripted(tmp_path_factory, True)
    assert eager['modes'] == ['eager1'] * len(eager['modes']) and not eager['captures']
    got = [m == 'graph' for m in replay['modes']]
    assert got == replay['expect'], [(i, m, e) for i, (m, e) in enumerate(zip(replay['modes'], replay['expect'])) if (m == 'graph') != e]
    assert all(m in ('graph', 'eager1') for m in replay['modes'])
    assert replay['kinds'] <= 16          # (Trainer.MAX_KINDS: no decision of the script was forgotten)
    # back on the first settings: a replay from the first call on, from a graph captured anew at that call
    first_back = replay['last_block']
    assert replay['expect'][first_back] and (first_back + 1) in replay['captures'], (first_back, replay['captures'])
    assert len(replay['captures']) >= replay['kinds'] + 1
    _same_bits(eager, replay, 'script')
