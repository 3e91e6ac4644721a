"""The yardstick of the combined-option tests is right and its statistic can see (no GPU): ComboOracleTrainer against the oracles the suite
already trusts, bit for bit; against tests/golden/sn_b.npz; the optimizer's identities in float64; the conditions on the case list; for
every modelled interaction error a case that separates it from the true oracle by 10 x the bound; and the committed noise table."""
import os

import numpy as np
import pytest
import torch

from oracle.patchgan_oracle import OracleTrainer
from tests import combo_util as C
from tests import spectral_util as S
from tests.ganloss_util import GanAugOracleTrainer, head_key
from tests.golden_util import LOSS_KEYS, Golden
from tests.segweight_util import WeightedSegOracleTrainer, weights_for

F64, F32 = torch.float64, torch.float32
_RUNS = {}


def _run(name, dtype=F64, mutate=None):
    """A case through its oracle, computed once and shared (never modified)."""
    key = (name, dtype, mutate)
    if key not in _RUNS:
        _RUNS[key] = C.run(name, dtype, mutate)
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------- 1. the case list
def test_at_most_ten_cases_on_the_fixtures_shapes():
    assert len(C.CASES) <= 10
    assert all(c['fixture'] in ('a_lrelu_tversky', 'b_tanh_wbce_norm', 'd_softmax_tversky') for c in C.CASES.values())
    assert all(c['accumulate'] in (None, 2, 3) for c in C.CASES.values()) and sum(c['accumulate'] == 3 for c in C.CASES.values()) == 1
    assert len({c['seed'] for c in C.CASES.values()}) == len(C.CASES)


def test_every_pair_of_levels_occurs_together():
    pairs = sum(len(C.FACTORS[a]) * len(C.FACTORS[b]) for a in C.FACTORS for b in C.FACTORS if a < b)
    missing = C.missing_pairs()
    print(f'pairwise coverage: {pairs - len(missing)} of {pairs} pairs of levels occur in the {len(C.CASES)} cases; missing: {missing}')
    for name, case in C.CASES.items():
        print(f'  {name:14s}', C.levels_of(case))
    assert not missing, missing
    # (the enumeration itself: dropping a case opens pairs again)
    assert C.missing_pairs({k: v for k, v in C.CASES.items() if k != C.EVERYTHING})


def test_one_case_has_every_factor_away_from_its_default():
    lv = C.levels_of(C.CASES[C.EVERYTHING])
    assert all(lv[f] != C.FACTORS[f][0] for f in C.FACTORS), lv
    assert all(v == C.FACTORS[f][0] for f, v in C.levels_of(C.CASES['plain']).items())


def test_diffaug_cases_take_both_ways_through_the_d_fake_pass():
    shared = {n: C.shares_dfake(n) for n, c in C.CASES.items() if c['diffaug']}
    print('diffaug cases, shared D(fake) pass:', shared)
    assert sum(shared.values()) >= 2 and sum(not v for v in shared.values()) >= 1, shared
    assert C.SHARED == {n: C.shares_dfake(n) for n in C.CASES}          # (what the GPU test expects to observe)


def test_hinge_cases_populate_both_sides_of_both_margins():
    names = [n for n, c in C.CASES.items() if c['gan'] == 'hinge']
    assert len(names) >= 2
    for n in names:
        sides = C.hinge_sides(_run(n)['first'])
        print(f'{n}: share of the real term below / above +1, of the fake term above / below -1:', sides)
        assert min(sides) >= 0.10, (n, sides)


def test_clip_cases_really_clip_the_first_update():
    names = [n for n, c in C.CASES.items() if c['clip'] is not None]
    assert names
    for n in names:
        f = _run(n)['first']
        print(f'{n}: coef gen {f["coef_g"]:.4f} disc {f["coef_d"]:.4f}')
        assert min(f['coef_g'], f['coef_d']) < 0.9, (n, f['coef_g'], f['coef_d'])


# ---------------------------------------------------------------------------------------------- 2. against the trusted oracles, bit for bit
def _same_run(a, b, x, y, steps=2, tables=None):
    for s in range(steps):
        if tables is not None:
            a.table = b.table = tables[s]
        la, lb = a.batch(x, y, train=True), b.batch(x, y, train=True)
        assert la == lb, (s, la, lb)
        for which in ('g_grads', 'd_grads'):
            assert list(a.last[which]) == list(b.last[which])
            assert all(torch.equal(a.last[which][k], b.last[which][k]) for k in b.last[which]), (s, which)
        for wa, wb in ((a.gw, b.gw), (a.dw, b.dw), (a.gm, b.gm), (a.gv, b.gv), (a.dm, b.dm), (a.dv, b.dv)):
            assert all(torch.equal(wa[k], wb[k]) for k in wb), s
    assert a.batch(x, y, train=False) == b.batch(x, y, train=False)
    assert (a.t_g, a.t_d) == (b.t_g, b.t_d) == (steps, steps)


def _fixture_args(gold):
    c = gold.cfg
    return dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=c['loss_type'])


@pytest.mark.parametrize('dtype', [F32, F64], ids=['float32', 'float64'])
@pytest.mark.parametrize('fixture', ['a_lrelu_tversky', 'b_tanh_wbce_norm'])
def test_every_option_at_its_default_is_oracle_trainer(fixture, dtype):
    gold = Golden(fixture)
    gw, dw = gold.weights('g0'), gold.weights('d0')
    a = C.ComboOracleTrainer(gw, dw, dtype=dtype, **_fixture_args(gold))
    b = OracleTrainer(gw, dw, dtype=dtype, **_fixture_args(gold))
    _same_run(a, b, *gold.inputs())


@pytest.mark.parametrize('dtype', [F32, F64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode,fa,r,gain', [('hinge', 'none', 1.0, 256.0), ('lsgan', 'sigmoid', 0.9, 1.0), ('vanilla', 'none', 0.9, 1.0)])
def test_gan_with_a_table_is_gan_aug_oracle_trainer(mode, fa, r, gain, dtype):
    gold = Golden('a_lrelu_tversky')
    gw, dw = gold.weights('g0'), gold.weights('d0')
    dw[head_key(dw)] = dw[head_key(dw)] * gain
    a = C.ComboOracleTrainer(gw, dw, dtype=dtype, gan_mode=mode, real_label=r, d_final_act=fa, **_fixture_args(gold))
    b = GanAugOracleTrainer(gw, dw, dtype=dtype, **_fixture_args(gold))
    b.gan_mode, b.real_label, b.d_final_act = mode, r, fa
    tables = [C.A.params_ref(9, s, 7, 0, 2, 256, 256) for s in range(2)]
    assert any(C.A.interesting(row, 256, 256) for t in tables for row in t)
    _same_run(a, b, *gold.inputs(), tables=tables)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['float32', 'float64'])
@pytest.mark.parametrize('fixture,loss_type', [('b_tanh_wbce_norm', 'focal+dice'), ('d_softmax_tversky', 'ce+dice'), ('a_lrelu_tversky', 'dice')])
def test_objectives_with_weights_are_weighted_seg_oracle_trainer(fixture, loss_type, dtype):
    gold = Golden(fixture)
    gw, dw = gold.weights('g0'), gold.weights('d0')
    args = dict(_fixture_args(gold), loss_type=loss_type)
    w = weights_for(gold.cfg['out_nc'])
    a = C.ComboOracleTrainer(gw, dw, dtype=dtype, class_weights=w, focal_gamma=3, focal_alpha=0.25, dice_smooth=0.5, **args)
    b = WeightedSegOracleTrainer(gw, dw, dtype=dtype, **args)
    b.focal_gamma, b.focal_alpha, b.dice_smooth, b.class_weights = 3, 0.25, 0.5, w
    _same_run(a, b, *gold.inputs())


# ---------------------------------------------------------------------------------------------- 3. spectral normalisation alone
def _sn_b_run(dtype):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sn_b.npz'))
    gold = Golden('a_lrelu_tversky')
    dsd = {k: torch.from_numpy(z['d0/' + k].copy()) for k in z['d0/keys']}
    o = C.ComboOracleTrainer(gold.weights('g0'), dsd, dtype=dtype, spectral=True, **_fixture_args(gold))
    x, y = gold.inputs()
    rows = np.array([[l[k] for k in LOSS_KEYS] for l in (o.batch(x, y, train=True) for _ in range(int(z['meta'][1])))])
    u_after = {k: v.clone() for k, v in o.su.items()}
    ev = o.batch(x, y, train=False)
    assert all(torch.equal(o.su[k], u_after[k]) for k in u_after)          # an evaluation call does not iterate
    return z, rows, np.array([[ev[k] for k in LOSS_KEYS]])


def test_spectral_alone_reproduces_the_fixture_in_float64():
    """Two float64 evaluations of one algorithm (the reference's modules under torch.nn.utils.spectral_norm with one power iteration per
    step, and ComboOracleTrainer): four training steps and an evaluation step to 1e-9 relative."""
    z, rows, ev = _sn_b_run(F64)
    for got, want in ((rows, z['losses64']), (ev, z['eval_losses64'][None])):
        err = np.abs(got - want) / np.abs(want)
        print('sn_b float64: largest relative difference', err.max())
        assert err.max() <= 1e-9, err


def test_spectral_alone_in_float32_stays_within_the_gpu_tests_bound():
    from tests.test_spectral_gpu import FLOOR_F, _bound
    z, rows, ev = _sn_b_run(F32)
    for what, got, w32, w64 in (('losses', rows, z['losses'], z['losses64']), ('eval', ev, z['eval_losses'][None], z['eval_losses64'][None])):
        for j, key in enumerate(LOSS_KEYS):
            err, bound = S.rel_dist(got[:, j], w64[:, j]), _bound(w32[:, j], w64[:, j], FLOOR_F)
            print(f'sn_b float32 {what} {key}: error {err:.3e} bound {bound:.3e}')
            assert err <= bound, (what, key, err, bound)


# ---------------------------------------------------------------------------------------------- 4. the optimizer's identities (float64)
def _plain(**over):
    return C.oracle('plain', F64, **over)


def _opt_state(o):
    out = {}
    for tag, d in (('gw', o.gw), ('dw', o.dw), ('gm', o.gm), ('gv', o.gv), ('dm', o.dm), ('dv', o.dv), ('ema', o.ema or {})):
        out.update({f'{tag}.{k}': v.detach().clone() for k, v in d.items()})
    return out


def test_a_window_of_one_batch_twice_is_one_plain_step():
    x, y = C.inputs('plain', 0)
    a, b = _plain(accumulate=2, ema_decay=0.99), _plain(ema_decay=0.99)
    la = [a.batch(x, y, train=True), a.batch(x, y, train=True)]
    lb = b.batch(x, y, train=True)
    assert la[0] == la[1] == lb and (a.t_g, a.t_d) == (1, 1)
    sa, sb = _opt_state(a), _opt_state(b)
    worst = max(float((sa[k] - sb[k]).abs().max() / sb[k].abs().max().clamp_min(1e-300)) for k in sb)
    print('accumulate = 2 on one batch twice against one step: largest relative difference', worst)
    assert worst <= 1e-12
    assert not torch.equal(sb['gw.' + next(iter(b.gw))], _opt_state(_plain())['gw.' + next(iter(b.gw))])


@pytest.mark.parametrize('over', [dict(clip_grad_norm=float('inf')), dict(weight_decay=0.0), dict(weight_decay=(0.0, None), clip_grad_norm=(None, float('inf')))],
                         ids=['clip-inf', 'decay-0', 'pairs'])
def test_an_infinite_max_norm_and_a_zero_decay_are_off_exactly(over):
    x, y = C.inputs('plain', 0)
    a, b = _plain(**over), _plain()
    for _ in range(2):
        assert a.batch(x, y, train=True) == b.batch(x, y, train=True)
    sa, sb = _opt_state(a), _opt_state(b)
    assert all(torch.equal(sa[k], sb[k]) for k in sb)
    if 'clip_grad_norm' in over:
        assert a.last['coef_d'] == 1.0


def test_a_nan_in_one_micro_batch_leaves_the_window_without_an_update():
    x, y = C.inputs('plain', 0)
    bad = x.clone()
    bad[0, 1, 17, 33] = float('nan')
    for first_bad in (True, False):
        # (least squares and MAE: torch's CPU nn.BCELoss refuses a NaN input outright, these carry it into both gradients)
        o = _plain(accumulate=2, clip_grad_norm=1.0, ema_decay=0.99, betas=C.OPTIM_BETAS, weight_decay=C.OPTIM_DECAY, gan_mode='lsgan', loss_type='MAE')
        before = _opt_state(o)
        o.batch(bad if first_bad else x, y, train=True)
        o.batch(x if first_bad else bad, y, train=True)
        after = _opt_state(o)
        assert all(bool(torch.isnan(whole).any()) for whole in (C.whole(o.last[n], o.last[n]) for n in ('g_grads', 'd_grads')))
        assert o.last['coef_g'] != o.last['coef_g'] and o.last['coef_d'] != o.last['coef_d']
        assert all(torch.equal(after[k], before[k]) for k in before)
        assert (o.t_g, o.t_d) == (1, 1)          # the step counts advance on a skipped update as well
        o.batch(x, y, train=True)
        o.batch(x, y, train=True)
        moved = _opt_state(o)
        assert (o.t_g, o.t_d) == (2, 2) and all(bool(torch.isfinite(v).all()) for v in moved.values())
        assert not torch.equal(moved['gw.' + next(iter(o.gw))], before['gw.' + next(iter(o.gw))])


# ---------------------------------------------------------------------------------------------- 5. the statistic can see
def _separation(mutation, name):
    r, true = _run(name, F64, mutation), _run(name)
    return C.separation(name, r['first'], r['losses'], r['state'], true, true)


def test_separation_table_names_every_mutation():
    assert set(C.SEPARATES) == set(C.MUTATIONS)
    assert all(case is None or C.mutation_applies(m, case) for m, case in C.SEPARATES.items())


@pytest.mark.parametrize('mutation', C.MUTATIONS)
def test_some_case_separates_the_mutation(mutation):
    """The float64 mutated oracle against the float64 true oracle, in units of 10 x the case's largest bound (>= 1 separates), over every
    case the mutation lives in; the case combo_util.SEPARATES records must separate.  Measured (the recorded case, its ratio):
    fake_other_row lsgan_ref 25, no_adjoint hinge_shared 88, sigma_before_iteration lsgan_sn 3e6, iterate_per_pass vanilla_ce 60,
    map_once_at_close everything 3.8, clip_per_call everything 95, decay_every_call everything 17, ema_every_call everything 10,
    mean_twice lsgan_sn 49, weights_skip_dice hinge_shared 260, real_label_on_gen lsgan_ref 8.9, stale_dfake hinge_sn_ref 5.8.
    decay_every_call and ema_every_call change a weight by lr x 1e-2, respectively 0.01 |w - ema|, per extra call: no case whose weights
    carry Adam's sign noise (a curve bound of 1e-3 .. 1e-1) reaches 0.2 for them.  `everything` clips to max-norms of 1e-8, which keeps
    Adam linear in the gradient and the bound at 9e-6, and gives the generator lr = 5e-2."""
    rows = [(name,) + _separation(mutation, name) for name in C.CASES if C.mutation_applies(mutation, name)]
    assert rows, mutation
    for name, s, sg, sc in rows:
        print(f'{mutation:24s} {name:14s} distance / (10 x bound): {s:12.3f}  (gradients {sg:.3f}, curve {sc:.3f})')
    best = max(rows, key=lambda r: r[1])
    want = C.SEPARATES[mutation]
    assert want is not None, f'no case separates {mutation}: the best is {best[0]} at {best[1]:.3f} of 10 x its bound'
    got = dict((r[0], r[1]) for r in rows)[want]
    assert got >= 1.0, (mutation, want, got)


# ---------------------------------------------------------------------------------------------- 6. the noise table
def test_committed_noise_table_is_the_float32_oracles_distance():
    bad = []
    assert set(C.COMBO_NOISE) == set(C.CASES)
    for name in C.CASES:
        r32, r64 = _run(name, F32), _run(name)
        grad = C.grad_dists(r32['first'], r64['first'])
        curve = max(C.curve_dist(r32['losses'], r32['state'], r64['losses'], r64['state']))
        kept = C.COMBO_NOISE[name]
        assert set(kept['grad']) == set(grad), name
        print(f"COMBO_NOISE[{name!r}]: curve {curve:.3e} (committed {kept['curve']:.3e}); gradients: largest {max(grad.values()):.3e} "
              f"(committed {max(kept['grad'].values()):.3e}), largest bound {C.largest_grad_bound(name):.3e}")
        for what, got, want in [('curve', curve, kept['curve'])] + [(k, grad[k], kept['grad'][k]) for k in grad]:
            if not want / 2 <= got <= want * 2:
                bad.append((name, what, got, want))
    assert not bad, bad
