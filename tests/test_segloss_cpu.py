"""The segmentation objectives beyond the reference's three, as far as they go without a device: tests/segloss_util.py's float64
references against torch autograd and torch's own losses, patchgan_amd.losses against the references, the plain fp32 evaluation within
the derived tolerances and every mutation outside them, linearity in the batch, the validator, the YAML and the argument checks of
pg_seg_loss_reduce / pg_seg_loss_value_grad (which precede any launch)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from tests import segloss_util as U

F64 = torch.float64
# (terms, focal_gamma, focal_alpha) of the kernel test
MASKS = [('ce', 2, None), ('focal', 0, None), ('focal', 2, None), ('focal', 5, None), ('focal', 0, 0.25), ('focal', 2, 0.25), ('focal', 5, 0.25),
         ('dice', 2, None), ('ce+dice', 2, None), ('focal+dice', 2, 0.25), ('ce+focal+dice', 2, 0.25)]
SHAPES = [(1, 1, 2), (2, 7, 3), (3, 900, 4), (40, 16, 8), (2, 33, 32)]


def _head(terms):
    return 'softmax' if 'ce' in terms else 'sigmoid'


def _inner(p):
    """The same tensor away from both clamps."""
    return p.clamp(2.0 ** -10, 1.0 - 2.0 ** -10)


# ---- the references ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_reference_gradient_is_autograd_of_the_value_away_from_the_clamps(terms, g, fa):
    for (N, HW, C), smooth in zip(SHAPES[:3], (1.0, 0.5, 3.0)):
        p, y = U.inputs(N, HW, C, _head(terms), 7 * N + HW)
        p = _inner(p)
        st = U.Settings(terms, g, fa, smooth, alpha=200.0, bglobal=2 * N)
        ref = U.reference(p, y, st)
        q = p.clone().requires_grad_(True)
        v = U.loss_of_p(q, y, st)
        dv, = torch.autograd.grad(v, q)
        assert abs(float(v.detach()) - ref['value']) <= 1e-13 * abs(ref['value'])
        assert float((dv - ref['grad']).abs().max()) <= 1e-11 * float(ref['grad'].abs().max())


def test_ce_is_nll_of_the_log_over_the_labelled_pixels():
    N, HW, C = 3, 900, 4
    p, y = U.inputs(N, HW, C, 'softmax', 5)
    p = _inner(p)
    labelled = y.sum(-1) > 0
    assert 0 < int(labelled.sum()) < N * HW
    labels = y.argmax(-1)
    want = F.nll_loss(torch.log(p)[labelled], labels[labelled], reduction='sum')
    st = U.Settings('ce', alpha=200.0)
    got = U.reference(p, y, st)['value'] * (N * HW) / 200.0
    assert abs(got - float(want)) <= 1e-13 * float(want)


def test_focal_with_gamma_0_and_no_alpha_is_binary_cross_entropy():
    for head, C in (('sigmoid', 1), ('sigmoid', 3), ('softmax', 4)):
        p, y = U.inputs(2, 33, C, head, 11)
        p = _inner(p)
        st = U.Settings('focal', 0, None, alpha=200.0)
        ref = U.reference(p, y, st)
        q = p.clone().requires_grad_(True)
        want = F.binary_cross_entropy(q, y) * 200.0
        dw, = torch.autograd.grad(want, q)
        assert abs(ref['value'] - float(want.detach())) <= 1e-13 * float(want.detach())
        assert float((ref['grad'] - dw).abs().max()) <= 1e-11 * float(dw.abs().max())


def test_an_empty_class_has_the_dice_coefficient_of_its_prediction_alone():
    p, y = U.inputs(2, 33, 3, 'softmax', 3)
    S = U.dice_sums(p, y)
    assert float(S[0, 2, 2]) == 0.0 and float(S[0, 2, 0]) == 0.0
    d = 1.0 - float(U.dice_of_sums(S[0:1, 2:3], 0.5))
    assert abs(d - 0.5 / (float(S[0, 2, 1]) + 0.5)) <= 1e-15


@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_losses_module_equals_the_references(terms, g, fa):
    """patchgan_amd.losses on NCHW tensors (planted values and clamps included) against the float64 references."""
    for N, HW, C in SHAPES[:3]:
        p, y = U.inputs(N, HW, C, _head(terms), N + HW)
        st = U.Settings(terms, g, fa, 0.75, alpha=200.0)
        nchw = lambda t: t.permute(0, 2, 1).reshape(N, C, HW, 1)
        got = float(U.seg_objective(terms, nchw(p), nchw(y), 200.0, g, fa, 0.75))
        want = U.reference(p, y, st)['value']
        assert abs(got - want) <= 1e-12 * abs(want), (terms, got, want)
    import patchgan.losses
    from patchgan_amd import losses
    assert patchgan.losses.dice_loss is losses.dice_loss and patchgan.losses.ce_loss is losses.ce_loss and patchgan.losses.focal_loss is losses.focal_loss
    for bad in (2.0, True, -1, 9):
        with pytest.raises(ValueError):
            losses.focal_loss(y, p, bad)


# ---- the plain fp32 evaluation and the mutations ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_plain_fp32_lies_within_the_tolerances(terms, g, fa):
    worst = (0.0, 0.0)
    shapes = SHAPES + ([(2, 33, 1)] if 'ce' not in terms else [])
    for N, HW, C in shapes:
        for smooth, ranks in ((1.0, 1), (0.5, 2)):
            p, y = U.inputs(N, HW, C, _head(terms), 1000 + N + HW + C)
            st = U.Settings(terms, g, fa, smooth, alpha=200.0, bglobal=ranks * N)
            value, grad = U.plain_fp32(p, y, st)
            rv, rg = U.ratios(p, y, st, value, grad)
            worst = (max(worst[0], rv), max(worst[1], rg))
            assert rv <= 1.0 and rg <= 1.0, (terms, g, fa, (N, HW, C), rv, rg)
    print(f'plain fp32 {terms} g={g} alpha={fa}: value {worst[0]:.3f}, gradient {worst[1]:.3f} of the bound')


def test_every_mutation_is_rejected():
    cases = {'dice_no_smooth_num': ('dice', 2, None), 'dice_k1_sign': ('ce+dice', 2, None), 'focal_no_g_term': ('focal+dice', 2, 0.25),
             'focal_swap_alpha': ('focal', 2, 0.25), 'ce_norm_chw': ('ce', 2, None), 'ce_no_clamp': ('ce+dice', 2, None)}
    assert set(cases) == set(U.MUTATIONS)
    for mut, (terms, g, fa) in cases.items():
        for N, HW, C in ((2, 7, 3), (3, 900, 4)):
            p, y = U.inputs(N, HW, C, _head(terms), 50 + HW)
            st = U.Settings(terms, g, fa, 1.0, alpha=200.0)
            rv, rg = U.ratios(p, y, st, *U.plain_fp32(p, y, st))
            assert rv <= 1.0 and rg <= 1.0
            mv, mg = U.ratios(p, y, st, *U.plain_fp32(p, y, st, mutate=mut))
            print(f'{mut} on {terms} ({N},{HW},{C}): value {mv:.3g}, gradient {mg:.3g} of the bound')
            assert not (mv <= 1.0 and mg <= 1.0), (mut, mv, mg)
            # the mutations that touch the gradient must show in it, not only in the value
            if mut in ('dice_k1_sign', 'focal_no_g_term', 'focal_swap_alpha', 'ce_norm_chw'):
                assert not mg <= 1.0, (mut, mg)


# ---- linearity in the batch ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_two_halves_of_a_batch_add_up_to_the_whole(terms, g, fa):
    """Every objective is a mean over samples: with Bglobal = 4 the values of the two halves add up to the whole batch's and their
    gradients are the whole's, in float64 to rounding."""
    N, HW, C = 4, 33, 3
    p, y = U.inputs(N, HW, C, _head(terms), 77)
    st = U.Settings(terms, g, fa, 1.0, alpha=200.0, bglobal=4)
    whole = U.reference(p, y, st)
    halves = [U.reference(p[h:h + 2], y[h:h + 2], st) for h in (0, 2)]
    assert abs(halves[0]['value'] + halves[1]['value'] - whole['value']) <= 4e-15 * abs(whole['value'])
    g2 = torch.cat([halves[0]['grad'], halves[1]['grad']])
    assert float((g2 - whole['grad']).abs().max()) <= 4e-15 * float(whole['grad'].abs().max())


# ---- the validator, the trainer and the YAML -------------------------------------------------------------------------------------------------

def test_the_validator_table():
    from patchgan_amd import _lib as L
    from patchgan_amd import engine as E
    assert E.SEG_OBJECTIVES == ('ce', 'focal', 'dice')
    for name in ('tversky', 'weighted_bce', 'MAE'):
        for head in ('sigmoid', 'softmax', 'tanh'):
            assert E.check_seg_loss(name, head, 1, 'x', 'y', None) is None          # not ours: the settings are inert
    bits = {'ce': L.SEG_CE, 'focal': L.SEG_FOCAL, 'dice': L.SEG_DICE}
    for k in (1, 2, 3):
        for members in itertools.permutations(E.SEG_OBJECTIVES, k):
            spec = E.check_seg_loss('+'.join(members), 'softmax', 4, 3, 0.25, 0.5)
            assert tuple(spec) == (sum(bits[m] for m in members), 3, 0.25, 0.5) and hash(spec) is not None
            assert (spec.terms, spec.focal_gamma, spec.focal_alpha, spec.dice_smooth) == tuple(spec)
    assert tuple(E.check_seg_loss('dice', 'sigmoid', 1)) == (L.SEG_DICE, 2, None, 1.0)
    assert tuple(E.check_seg_loss('focal+dice', 'sigmoid', 1, 0, None, 2)) == (L.SEG_FOCAL | L.SEG_DICE, 0, None, 2.0)
    with pytest.raises(ValueError) as info:
        E.check_seg_loss('jaccard', 'softmax', 4)
    assert all(n in str(info.value) for n in ('tversky', 'weighted_bce', 'MAE', 'ce', 'focal', 'dice'))
    bad = [('ce+ce', 'softmax', 4), ('dice+tversky', 'softmax', 4), ('tversky+MAE', 'softmax', 4), ('MAE+ce', 'softmax', 4), ('', 'softmax', 4),
           ('ce+', 'softmax', 4), ('Dice', 'softmax', 4), (None, 'softmax', 4), (3, 'softmax', 4), (('ce',), 'softmax', 4), ('ce dice', 'softmax', 4),
           ('ce', 'sigmoid', 4), ('ce+dice', 'sigmoid', 4), ('ce', 'softmax', 1), ('ce', 'tanh', 4), ('dice', 'tanh', 1), ('focal', 'none', 1),
           ('focal+dice', 'relu', 2), ('dice', None, 1)]
    for args in bad:
        with pytest.raises(ValueError):
            E.check_seg_loss(*args)
    for kw in (dict(focal_gamma=2.0), dict(focal_gamma=True), dict(focal_gamma=-1), dict(focal_gamma=9), dict(focal_gamma='2'), dict(focal_gamma=None),
               dict(focal_alpha=0), dict(focal_alpha=1), dict(focal_alpha=1.0), dict(focal_alpha=-0.25), dict(focal_alpha=True), dict(focal_alpha='0.25'),
               dict(focal_alpha=float('nan')), dict(focal_alpha=1e-50), dict(dice_smooth=0), dict(dice_smooth=-1.0), dict(dice_smooth=float('inf')),
               dict(dice_smooth=float('nan')), dict(dice_smooth=None), dict(dice_smooth=True), dict(dice_smooth='1'), dict(dice_smooth=1e-60),
               dict(dice_smooth=1e60)):
        for name in ('dice', 'focal', 'ce+focal+dice'):          # (checked whichever member is selected)
            with pytest.raises(ValueError):
                E.check_seg_loss(name, 'softmax', 4, **kw)


def _trainer(tmp_path, final_act='sigmoid', C=1):
    import patchgan_amd as pg
    g = pg.UNet(3, C, 4, use_dropout=False, activation='leakyrelu', final_act=final_act)
    d = pg.Discriminator(3 + C, 4, n_layers=3)
    return pg.Trainer(g, d, str(tmp_path))


def test_trainer_validation_comes_before_any_launch(tmp_path):
    import patchgan_amd as pg
    assert (pg.Trainer.focal_gamma, pg.Trainer.focal_alpha, pg.Trainer.dice_smooth) == (2, None, 1.0)
    x = torch.zeros(2, 3, 256, 256)
    cases = [('sigmoid', 1, dict(loss_type='ce')), ('sigmoid', 1, dict(loss_type='jaccard')), ('softmax', 4, dict(loss_type='ce+MAE')),
             ('softmax', 4, dict(loss_type='dice+dice')), ('sigmoid', 1, dict(loss_type='focal', focal_gamma=2.5)),
             ('sigmoid', 1, dict(loss_type='focal', focal_alpha=1.5)), ('sigmoid', 1, dict(loss_type='dice', dice_smooth=0.0)),
             ('softmax', 4, dict(loss_type='ce+dice', dice_smooth=-1))]
    for fa, C, attrs in cases:
        t = _trainer(tmp_path, fa, C)
        for k, v in attrs.items():
            setattr(t, k, v)
        for train in (True, False):
            with pytest.raises(ValueError):          # (CPU tensors: anything later than the check would raise RuntimeError instead)
                t.batch(x, x[:, :1].expand(2, C, 256, 256), train=train)
        with pytest.raises(ValueError):
            t.evaluate([(x, x[:, :1].expand(2, C, 256, 256))])
    for fa, C, attrs in (('sigmoid', 1, dict(loss_type='dice')), ('sigmoid', 1, dict(loss_type='focal+dice', focal_alpha=0.25)),
                         ('softmax', 4, dict(loss_type='ce+dice')), ('softmax', 4, dict(loss_type='ce+focal+dice', focal_gamma=0)),
                         ('sigmoid', 1, dict(loss_type='tversky', focal_gamma='inert', dice_smooth=-5))):
        t = _trainer(tmp_path, fa, C)
        for k, v in attrs.items():
            setattr(t, k, v)
        with pytest.raises(RuntimeError):            # valid settings: the step gets as far as asking for a HIP device
            t.batch(x, x[:, :1].expand(2, C, 256, 256), train=True)


def test_kind_key_gains_the_settings_only_with_a_new_objective(tmp_path):
    x = torch.zeros(2, 3, 256, 256)
    args = (x, x[:, :1], False, (2, 256, 256, 3, 1))
    t = _trainer(tmp_path)
    t.setup_optimizers()
    off = t._kind_key(*args, True)
    t.focal_gamma, t.focal_alpha, t.dice_smooth = 5, 0.25, 0.5
    assert t._kind_key(*args, True) == off and t._seg_key() == () and t._seg_now() is None
    for lt in ('weighted_bce', 'MAE'):
        t.loss_type = lt
        assert t._seg_key() == () and len(t._kind_key(*args, True)) == len(off)
    keys = {off}
    for lt, g, fa, s in (('dice', 2, None, 1.0), ('dice', 2, None, 0.5), ('focal', 2, None, 1.0), ('focal', 5, None, 1.0), ('focal', 5, 0.25, 1.0),
                         ('focal+dice', 5, 0.25, 1.0)):
        t.loss_type, t.focal_gamma, t.focal_alpha, t.dice_smooth = lt, g, fa, s
        for train in (True, False):
            k = t._kind_key(*args, train)
            assert k not in keys and ('seg', t._seg_now().terms, g, fa, s) in k
            keys.add(k)


TRAIN_YAML = """
train_params:
  loss_type: %s
  seg_alpha: 200
%s
"""


def test_yaml_settings(tmp_path):
    from patchgan_amd.train import apply_train_params, seg_loss_of
    tp = lambda lt, text='': yaml.safe_load(TRAIN_YAML % (lt, text))['train_params']
    assert seg_loss_of(tp('tversky'), 'sigmoid', 1) == (2, None, 1.0)
    assert seg_loss_of(tp('ce+dice', '  focal_gamma: 3\n  focal_alpha: 0.25\n  dice_smooth: 0.5'), 'softmax', 4) == (3, 0.25, 0.5)
    assert seg_loss_of(tp('focal', '  focal_alpha: null\n  focal_gamma: 0'), 'sigmoid', 1) == (0, None, 1.0)
    t = _trainer(tmp_path)
    apply_train_params(t, tp('focal+dice', '  focal_gamma: 4\n  dice_smooth: 2'))
    assert (t.loss_type, t.focal_gamma, t.focal_alpha, t.dice_smooth) == ('focal+dice', 4, None, 2)
    apply_train_params(t, tp('tversky'))
    assert (t.loss_type, t.focal_gamma, t.focal_alpha, t.dice_smooth) == ('tversky', 2, None, 1.0)
    for lt, text in (('ce', ''), ('dice', '  dice_smooth: 0'), ('focal', '  focal_gamma: 2.5'), ('focal', '  focal_gamma: true'),
                     ('focal', '  focal_alpha: 1'), ('dice+MAE', ''), ('lovasz', '')):
        with pytest.raises(ValueError):
            apply_train_params(t, tp(lt, text))


def test_patchgan_train_refuses_a_bad_objective_before_any_network_is_built(tmp_path, monkeypatch):
    """The CLI reads the YAML, then checks the objective against the generator's head and channel count; no data set and no network
    exists yet (their constructors are replaced by ones that fail the test)."""
    import patchgan_amd.train as T
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_: None)

    def never(*a, **k):
        raise AssertionError('built before the objective was checked')
    for name in ('UNet', 'Discriminator', 'Trainer', 'load_plugin_dataset', 'COCOStuffDataset'):
        monkeypatch.setattr(T, name, never)
    base = {'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 4,
                        'train_data': {'images': '4', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
            'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'final_activation': 'softmax'},
                             'discriminator': {'filters': 4, 'n_layers': 3}},
            'checkpoint_path': str(tmp_path / 'ckpt')}
    tp = {'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3}
    bad = [dict(loss_type='ce+ce'), dict(loss_type='jaccard'), dict(loss_type='focal', focal_gamma=1.5), dict(loss_type='dice', dice_smooth=0),
           dict(loss_type='focal+dice', focal_alpha=2)]
    for extra in bad:
        (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(dict(base, train_params=dict(tp, **extra))))
        with pytest.raises(ValueError):
            T.patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])
    # 'ce' on a sigmoid head, and on one channel
    for fa, C in (('sigmoid', 4), ('softmax', 1)):
        cfg = dict(base, train_params=dict(tp, loss_type='ce'))
        cfg['model_params'] = {'generator': {'filters': 4, 'activation': 'leakyrelu', 'final_activation': fa}, 'discriminator': {'filters': 4, 'n_layers': 3}}
        cfg['dataset'] = dict(base['dataset'], out_channels=C)
        (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
        with pytest.raises(ValueError):
            T.patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])
    # a good one passes the check and reaches the first constructor
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(dict(base, train_params=dict(tp, loss_type='ce+dice'))))
    with pytest.raises(AssertionError, match='built before'):
        T.patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])


# ---- the C ABI's argument checks (no launch is reached: these run without a device) -----------------------------------------------------------

def test_argument_errors_before_any_launch():
    from patchgan_amd import _lib as L
    lib = L.load()
    N, HW, C = 2, 4096, 4
    need = lib.pg_seg_loss_workspace_bytes(N, HW, C)
    assert lib.pg_seg_loss_slabs(N, HW) == 4 and need == N * 4 * C * 5 * 8
    assert [lib.pg_seg_loss_slabs(1, hw) for hw in (1, 2047, 2048, 65536, 1 << 20)] == [1, 1, 2, 64, 128]
    assert lib.pg_seg_loss_slabs(8, 512 * 512) == 128 and lib.pg_seg_loss_slabs(40, 1 << 20) == 25 and lib.pg_seg_loss_slabs(5000, 1 << 20) == 1
    for bad in ((0, HW, C), (N, 0, C), (N, HW, 0), (-1, HW, C)):
        assert lib.pg_seg_loss_workspace_bytes(*bad) == 0
    assert lib.pg_seg_loss_slabs(0, HW) == 0 and lib.pg_seg_loss_slabs(N, 0) == 0
    P, Y, G, V, WS = 4096, 1 << 20, 1 << 21, 1 << 22, 1 << 23          # (never dereferenced: every call below is refused)
    ok = dict(p=P, ld_p=8, y=Y, ld_y=8, N=N, HW=HW, C=C, terms=L.SEG_CE | L.SEG_DICE, gamma=2, fa=L.SEG_FOCAL_ALPHA_NONE, smooth=1.0,
              ws=WS, nb=need, g=G, ld_g=4, value=V)

    def reduce(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_reduce(a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'], a['fa'], a['ws'], a['nb'], None)

    def finish(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_value_grad(a['ws'], a['nb'], a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'],
                                          a['fa'], a['smooth'], 0.1, 0.1, 0.1, a['g'], a['ld_g'], a['value'], None)
    both = [dict(p=None), dict(y=None), dict(ws=None), dict(ws=WS + 4), dict(nb=need - 8), dict(nb=0), dict(N=0), dict(N=-2), dict(HW=0), dict(C=0),
            dict(C=-1), dict(ld_p=3), dict(ld_y=3), dict(terms=0), dict(terms=8), dict(terms=L.SEG_CE | 16), dict(terms=-1),
            dict(terms=L.SEG_CE, C=1, ld_p=1, ld_y=1), dict(terms=L.SEG_CE | L.SEG_FOCAL, C=1), dict(gamma=-1), dict(gamma=9), dict(fa=0.0), dict(fa=1.0),
            dict(fa=-0.5), dict(fa=1.5), dict(fa=float('nan')), dict(fa=float('inf'))]
    for kw in both:
        assert reduce(**kw) == -1, kw
        assert finish(**kw) == -1, kw
    for kw in (dict(value=None), dict(ld_g=3), dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float('inf')), dict(smooth=float('nan'))):
        assert finish(**kw) == -1, kw
