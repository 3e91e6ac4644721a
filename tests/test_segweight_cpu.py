"""Per-class weights of the segmentation objectives without a GPU (Trainer.class_weights): the validator, the trainer's and the CLI's
checks, weights from counts, the torch ops of patchgan_amd.losses against torch's own weighted losses in float64, the weighted
tolerances of tests/segweight_util.py (the plain-fp32 evaluation inside them, three planted mutations outside) and the argument
checks of the two new entry points."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from tests import segloss_util as U
from tests import segweight_util as WU

MASKS = [('ce', 2, None), ('focal', 0, None), ('focal', 2, 0.25), ('dice', 2, None), ('ce+dice', 2, None), ('focal+dice', 2, 0.25),
         ('ce+focal+dice', 2, 0.25)]
SHAPES = [(1, 1, 2), (2, 7, 3), (3, 900, 4), (40, 16, 8), (2, 33, 32)]


def _head(terms):
    return 'softmax' if 'ce' in terms else 'sigmoid'


# ---- the validator ---------------------------------------------------------------------------------------------------------------------------

def test_the_validator_takes_weights():
    from patchgan_amd import engine as E
    plain = E.check_seg_loss('ce+dice', 'softmax', 4)
    assert len(plain) == 4 and plain.class_weights is None and plain.cw is None
    assert E.check_seg_loss('ce+dice', 'softmax', 4, class_weights=None) == plain
    spec = E.check_seg_loss('ce+dice', 'softmax', 4, class_weights=[0.1, 37.5, 0, 1])
    f = lambda v: float(np.float32(v))
    assert spec.class_weights == (f(0.1), 37.5, 0.0, 1.0) and tuple(spec)[:4] == tuple(plain) and spec != plain
    assert hash(spec) == hash(E.check_seg_loss('ce+dice', 'softmax', 4, class_weights=(0.1, 37.5, 0.0, 1.0)))
    assert spec != E.check_seg_loss('ce+dice', 'softmax', 4, class_weights=[0.1, 37.5, 0, 2])
    assert E.check_seg_loss('dice', 'sigmoid', 2, class_weights=np.array([1.0, 2.0], dtype=np.float32)).class_weights == (1.0, 2.0)
    assert E.check_seg_loss('focal', 'sigmoid', 1, class_weights=[3]).class_weights == (3.0,)
    bad = [[1, 2, 3], [1, 2, 3, 4, 5], [], [1, 2, 3, -1], [1, 2, 3, float('nan')], [1, 2, 3, float('inf')], [0, 0, 0, 0], [1, 2, 3, 1e60],
           [1e-60, 0, 0, 0], [1, 2, 3, '4'], [1, 2, 3, None], [1, 2, 3, True], 'balanced', 'balanced_sqrt', 'inverse', 1.0, [[1, 2, 3, 4]]]
    for w in bad:
        with pytest.raises(ValueError):
            E.check_seg_loss('ce+dice', 'softmax', 4, class_weights=w)
    # one of the reference's three objectives has no per-class weights: anything but None is refused, not silently inert
    for name in ('tversky', 'weighted_bce', 'MAE'):
        assert E.check_seg_loss(name, 'sigmoid', 1, class_weights=None) is None
        for w in ([1.0], [1, 2, 3, 4], 'balanced'):
            with pytest.raises(ValueError):
                E.check_seg_loss(name, 'sigmoid', 1, class_weights=w)


def _trainer(tmp_path, final_act='softmax', C=4):
    import patchgan_amd as pg
    g = pg.UNet(3, C, 4, use_dropout=False, activation='leakyrelu', final_act=final_act)
    d = pg.Discriminator(3 + C, 4, n_layers=3)
    return pg.Trainer(g, d, str(tmp_path))


def test_trainer_validation_comes_before_any_launch(tmp_path):
    import patchgan_amd as pg
    assert pg.Trainer.class_weights is None and pg.Trainer.class_weight_batches is None
    x = torch.zeros(2, 3, 256, 256)
    y = x[:, :1].expand(2, 4, 256, 256)
    bad = [dict(loss_type='ce+dice', class_weights=[1, 2, 3]), dict(loss_type='ce+dice', class_weights=[1, 2, 3, -4]),
           dict(loss_type='dice', class_weights=[0, 0, 0, 0]), dict(loss_type='ce', class_weights='balanced'),
           dict(loss_type='ce', class_weights='balanced_sqrt'), dict(loss_type='ce', class_weights='median'),
           dict(loss_type='tversky', class_weights=[1, 2, 3, 4]), dict(loss_type='MAE', class_weights='balanced'),
           dict(loss_type='weighted_bce', class_weights=[1, 1, 1, 1])]
    for attrs in bad:
        t = _trainer(tmp_path)
        for k, v in attrs.items():
            setattr(t, k, v)
        for train in (True, False):
            with pytest.raises(ValueError):          # (CPU tensors: anything later than the check would raise RuntimeError instead)
                t.batch(x, y, train=train)
        with pytest.raises(ValueError):
            t.evaluate([(x, y)])
    for attrs in (dict(loss_type='ce+dice', class_weights=[0.1, 37.5, 0, 1]), dict(loss_type='focal', class_weights=(1, 1, 1, 1)),
                  dict(loss_type='tversky', class_weights=None)):
        t = _trainer(tmp_path)
        for k, v in attrs.items():
            setattr(t, k, v)
        with pytest.raises(RuntimeError):            # valid settings: the step gets as far as asking for a HIP device
            t.batch(x, y, train=True)
    t = _trainer(tmp_path)
    for args in (dict(scheme='median'), dict(max_batches=0), dict(max_batches=2.5)):
        with pytest.raises(ValueError):
            t.estimate_class_weights([(x, y)], **args)
    with pytest.raises(ValueError):
        _trainer(tmp_path, 'sigmoid', 1).estimate_class_weights([(x, y[:, :1])])
    # train() with a scheme beside one of the reference's three objectives: refused before any pass over the data

    def never():
        raise AssertionError('the data was read before the setting was checked')
        yield
    t = _trainer(tmp_path)
    t.loss_type, t.class_weights = 'tversky', 'balanced'
    with pytest.raises(ValueError):
        t.train(never(), [], 1)


def test_kind_key_gains_the_weights_only_when_they_are_set(tmp_path):
    x = torch.zeros(2, 3, 256, 256)
    args = (x, x[:, :1].expand(2, 4, 256, 256), False, (2, 256, 256, 3, 4))
    t = _trainer(tmp_path)
    t.loss_type = 'ce+dice'
    t.setup_optimizers()
    off = t._kind_key(*args, True)
    bare = _trainer(tmp_path)
    bare.loss_type = 'ce+dice'
    bare.setup_optimizers()
    assert t._seg_key() == bare._seg_key() and len(t._seg_key()[0]) == 5          # ('seg', terms, gamma, alpha, smooth)
    keys = {off}
    for w in ([1, 1, 1, 1], [0.1, 37.5, 0, 1], [0.1, 37.5, 0, 2]):
        t.class_weights = w
        for train in (True, False):
            k = t._kind_key(*args, train)
            assert k not in keys and t._seg_key()[0][-1] == tuple(float(np.float32(v)) for v in w)
            keys.add(k)
    t.class_weights = None
    assert t._kind_key(*args, True) == off


TRAIN_YAML = """
train_params:
  loss_type: %s
  seg_alpha: 200
%s
"""


def test_yaml_settings(tmp_path):
    from patchgan_amd.train import apply_train_params, class_weights_of
    tp = lambda lt, text='': yaml.safe_load(TRAIN_YAML % (lt, text))['train_params']
    assert class_weights_of(tp('tversky'), 'sigmoid', 1) == (None, None)
    assert class_weights_of(tp('ce+dice'), 'softmax', 4) == (None, None)
    assert class_weights_of(tp('ce+dice', '  class_weights: [0.1, 37.5, 0, 1]'), 'softmax', 4) == ([0.1, 37.5, 0, 1], None)
    assert class_weights_of(tp('ce+dice', '  class_weights: balanced\n  class_weight_batches: 8'), 'softmax', 4) == ('balanced', 8)
    assert class_weights_of(tp('focal', '  class_weights: balanced_sqrt'), 'sigmoid', 3) == ('balanced_sqrt', None)
    t = _trainer(tmp_path)
    apply_train_params(t, tp('ce+dice', '  class_weights: balanced\n  class_weight_batches: 3'))
    assert (t.loss_type, t.class_weights, t.class_weight_batches) == ('ce+dice', 'balanced', 3)
    apply_train_params(t, tp('dice', '  class_weights: [1, 2, 3, 4]'))
    assert (t.class_weights, t.class_weight_batches) == ([1, 2, 3, 4], None)
    apply_train_params(t, tp('tversky'))
    assert (t.class_weights, t.class_weight_batches) == (None, None)
    for lt, text in (('ce+dice', '  class_weights: [1, 2, 3]'), ('ce+dice', '  class_weights: [1, 2, 3, -1]'), ('dice', '  class_weights: median'),
                     ('dice', '  class_weights: 2.0'), ('tversky', '  class_weights: [1, 2, 3, 4]'), ('MAE', '  class_weights: balanced'),
                     ('dice', '  class_weights: balanced\n  class_weight_batches: 0'), ('dice', '  class_weights: balanced\n  class_weight_batches: 1.5'),
                     ('dice', '  class_weight_batches: 4'), ('dice', '  class_weights: [1, 2, 3, 4]\n  class_weight_batches: 4')):
        with pytest.raises(ValueError):
            apply_train_params(t, tp(lt, text))
    with pytest.raises(ValueError):          # a scheme on one channel
        class_weights_of(tp('dice', '  class_weights: balanced'), 'sigmoid', 1)


def test_patchgan_train_refuses_bad_weights_before_any_network_is_built(tmp_path, monkeypatch):
    """The CLI reads the YAML, then checks the weights with the objective against the generator's head and channel count; no data set
    and no network exists yet (their constructors are replaced by ones that fail the test)."""
    import patchgan_amd.train as T
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_: None)

    def never(*a, **k):
        raise AssertionError('built before the weights were checked')
    for name in ('UNet', 'Discriminator', 'Trainer', 'load_plugin_dataset', 'COCOStuffDataset'):
        monkeypatch.setattr(T, name, never)
    base = {'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 4,
                        'train_data': {'images': '4', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
            'model_params': {'generator': {'filters': 4, 'activation': 'leakyrelu', 'final_activation': 'softmax'},
                             'discriminator': {'filters': 4, 'n_layers': 3}},
            'checkpoint_path': str(tmp_path / 'ckpt')}
    tp = {'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3}
    run = lambda: T.patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])
    bad = [dict(loss_type='ce+dice', class_weights=[1, 2, 3]), dict(loss_type='ce+dice', class_weights=[1, 2, 3, -1]),
           dict(loss_type='ce+dice', class_weights=[0, 0, 0, 0]), dict(loss_type='dice', class_weights='median'),
           dict(loss_type='tversky', class_weights=[1, 2, 3, 4]), dict(loss_type='weighted_bce', class_weights='balanced'),
           dict(loss_type='dice', class_weights='balanced', class_weight_batches=0)]
    for extra in bad:
        (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(dict(base, train_params=dict(tp, **extra))))
        with pytest.raises(ValueError):
            run()
    for extra in (dict(loss_type='ce+dice', class_weights=[0.1, 37.5, 0, 1]), dict(loss_type='ce+dice', class_weights='balanced', class_weight_batches=4)):
        (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(dict(base, train_params=dict(tp, **extra))))
        with pytest.raises(AssertionError, match='built before'):
            run()


# ---- weights from counts ---------------------------------------------------------------------------------------------------------------------

def test_class_weights_from_counts_by_hand():
    from patchgan_amd.engine import class_weights_from_counts as cwc
    f = lambda vs: [float(np.float32(v)) for v in vs]
    # f = (1/2, 1/4, 1/4): r = (2, 4, 4), sum 10, w = r * 3 / 10
    assert cwc([2, 1, 1], 'balanced') == f([0.6, 1.2, 1.2])
    # f = (1/4, 3/4) ... sqrt: r = (2, 2 / sqrt 3), w = r * 2 / sum r
    r = np.array([2.0, 2.0 / np.sqrt(3.0)])
    assert cwc([25, 75], 'balanced_sqrt') == f(r * 2 / r.sum())
    # equal counts: all ones, whatever the scheme and the total
    assert cwc([7, 7, 7, 7], 'balanced') == [1.0] * 4 and cwc([10 ** 12] * 5, 'balanced_sqrt') == [1.0] * 5
    # a class that does not occur takes the largest r among those that do: f = (0.9, 0.1, -): r = (10/9, 10, 10)
    r = np.array([10.0 / 9.0, 10.0, 10.0])
    assert cwc([90, 10, 0], 'balanced') == f(r * 3 / r.sum())
    r = np.array([1 / np.sqrt(0.9), 1 / np.sqrt(0.1), 1 / np.sqrt(0.1)])
    assert cwc([90, 10, 0], 'balanced_sqrt') == f(r * 3 / r.sum())
    # the mean is 1 to fp32 rounding; a 1 % class counts ~ 99 / 2 times the rest per pixel
    w = cwc([99, 1])
    assert abs(sum(w) / 2 - 1) < 1e-6 and abs(w[1] / w[0] - 99) < 1e-4
    for bad in ([5], [], [0, 0, 0], [3, -1]):
        with pytest.raises(ValueError):
            cwc(bad, 'balanced')
    with pytest.raises(ValueError):
        cwc([1, 2], 'median')
    assert cwc(np.array([2, 1, 1], dtype=np.uint64)) == f([0.6, 1.2, 1.2])


def test_label_counts_of_the_utility():
    y = np.array([[[1, 0, 0], [0.5, 0.5, 0], [0.4999, 0, 0], [float('nan'), 0, 1], [0, 0, 0]]], dtype=np.float32)
    assert WU.label_counts(y).tolist() == [2, 1, 1, 2, 5]
    y = WU.count_target(2, 33, 4, 1).numpy()
    c = WU.label_counts(y)
    assert c[-1] == 66 and np.isnan(y).sum() >= 2 and c[4] > 0


# ---- the torch ops in float64 ----------------------------------------------------------------------------------------------------------------

def _nchw(t, H=None):
    N, HW, C = t.shape
    H = H or 1
    return t.permute(0, 2, 1).reshape(N, C, H, HW // H).contiguous()


def test_ce_is_torchs_weighted_cross_entropy_with_the_sum_over_the_pixel_count():
    from patchgan_amd import losses
    N, H, W, C = 3, 5, 7, 4
    gen = torch.Generator().manual_seed(3)
    logits = torch.rand(N, C, H, W, generator=gen, dtype=torch.float64) * 8 - 4          # (away from the clamps)
    labels = torch.randint(0, C, (N, H, W), generator=gen)
    w = torch.tensor(WU.weights_for(C), dtype=torch.float64)
    y = F.one_hot(labels, C).permute(0, 3, 1, 2).double()
    got = losses.ce_loss(y, torch.softmax(logits, 1), class_weights=w)
    want = F.cross_entropy(logits, labels, weight=w, reduction='sum') / (N * H * W)
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
    # ... which is not torch's weighted mean (that one divides by the weights of the labelled pixels)
    mean = F.cross_entropy(logits, labels, weight=w, reduction='mean')
    assert abs(float(mean) * float(w[labels].sum()) / (N * H * W) - float(want)) <= 1e-13 * abs(float(want))
    assert abs(float(mean) - float(want)) > 1e-3 * abs(float(want))
    assert abs(float(losses.ce_loss(y, torch.softmax(logits, 1), class_weights=WU.weights_for(C))) - float(want)) <= 1e-13 * abs(float(want))


def test_focal_with_gamma_0_is_torchs_weighted_binary_cross_entropy():
    from patchgan_amd import losses
    N, H, W, C = 2, 6, 5, 3
    gen = torch.Generator().manual_seed(4)
    p = torch.sigmoid(torch.rand(N, C, H, W, generator=gen, dtype=torch.float64) * 8 - 4)
    y = (torch.rand(N, C, H, W, generator=gen) < 0.3).double()
    w = torch.tensor(WU.weights_for(C), dtype=torch.float64)
    got = losses.focal_loss(y, p, gamma=0, class_weights=w)
    want = F.binary_cross_entropy(p, y, weight=w.view(1, C, 1, 1).expand_as(p))
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))


def test_dice_against_an_explicit_loop():
    from patchgan_amd import losses
    N, H, W, C = 3, 4, 5, 4
    gen = torch.Generator().manual_seed(5)
    p = torch.rand(N, C, H, W, generator=gen, dtype=torch.float64)
    y = (torch.rand(N, C, H, W, generator=gen) < 0.3).double()
    w = WU.weights_for(C)
    for smooth in (1.0, 0.5):
        want = 0.0
        for n in range(N):
            for c in range(C):
                i, ps, ys = float((p[n, c] * y[n, c]).sum()), float(p[n, c].sum()), float(y[n, c].sum())
                want += w[c] * (1.0 - (2.0 * i + smooth) / (ps + ys + smooth))
        want /= N * C
        got = losses.dice_loss(y, p, smooth, class_weights=w)
        assert abs(float(got) - want) <= 1e-13 * abs(want)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_all_ones_equal_the_unweighted_call_exactly(dtype):
    from patchgan_amd import losses
    p, y = U.inputs(3, 35, 4, 'softmax', 6)
    p, y = _nchw(p, 5).to(dtype), _nchw(y, 5).to(dtype)
    ones = [1.0] * 4
    assert torch.equal(losses.ce_loss(y, p), losses.ce_loss(y, p, class_weights=ones))
    assert torch.equal(losses.ce_loss(y, p), losses.ce_loss(y, p, class_weights=None))
    for g, fa in ((0, None), (2, 0.25)):
        assert torch.equal(losses.focal_loss(y, p, g, fa), losses.focal_loss(y, p, g, fa, class_weights=ones))
    assert torch.equal(losses.dice_loss(y, p, 0.5), losses.dice_loss(y, p, 0.5, class_weights=torch.ones(4, dtype=dtype)))
    with pytest.raises(ValueError):
        losses.dice_loss(y, p, class_weights=[1, 2, 3])


@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_losses_module_equals_the_weighted_references(terms, g, fa):
    """The torch ops of patchgan_amd.losses, the weighted float64 reference of tests/segweight_util.py and float64 autograd of its
    value agree (away from the clamps for the gradient)."""
    N, H, W, C = 2, 3, 11, 3
    p, y = U.inputs(N, H * W, C, _head(terms), 70)
    p = p.clamp(1e-3, 1 - 1e-3)
    w = WU.weights_for(C)
    st = U.Settings(terms, g, fa, 0.5, alpha=200.0)
    ref = WU.reference(p, y, st, w)
    got = WU.seg_objective(terms, _nchw(p, H), _nchw(y, H), 200.0, g, fa, 0.5, class_weights=w)
    assert abs(float(got) - ref['value']) <= 1e-12 * abs(ref['value'])
    q = p.clone().requires_grad_(True)
    auto, = torch.autograd.grad(WU.loss_of_p(q, y, st, w), q)
    assert float((auto - ref['grad']).abs().max()) <= 1e-12 * float(ref['grad'].abs().max())
    # all ones: the unweighted reference
    one = WU.reference(p, y, st, [1.0] * C)
    plain = U.reference(p, y, st)
    assert one['value'] == plain['value'] and torch.equal(one['grad'], plain['grad'])


# ---- the tolerances --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms,g,fa', MASKS)
def test_plain_fp32_lies_within_the_weighted_tolerances(terms, g, fa):
    worst = (0.0, 0.0)
    for N, HW, C in SHAPES:
        for smooth, ranks in ((1.0, 1), (0.5, 2)):
            p, y = U.inputs(N, HW, C, _head(terms), 1000 + N + HW + C)
            w = WU.weights_for(C)
            st = U.Settings(terms, g, fa, smooth, alpha=200.0, bglobal=ranks * N)
            value, grad = WU.plain_fp32(p, y, st, w)
            rv, rg = WU.Expect(p, y, st, w).ratios(value, grad)
            worst = (max(worst[0], rv), max(worst[1], rg))
            assert rv <= 1.0 and rg <= 1.0, (terms, g, fa, (N, HW, C), rv, rg)
            zero = [c for c in range(C) if w[c] == 0.0]
            assert np.all(grad[..., zero] == 0.0)
    print(f'weighted plain fp32 {terms} g={g} alpha={fa}: value {worst[0]:.3f}, gradient {worst[1]:.3f} of the bound')


def test_weighted_tolerances_with_all_ones_are_the_unweighted_ones():
    p, y = U.inputs(3, 900, 4, 'softmax', 12)
    st = U.Settings('ce+focal+dice', 2, 0.25, 1.0, alpha=200.0)
    tv, tg = WU.tolerances(p, y, st, [1.0] * 4)
    uv, ug = U.tolerances(p, y, st)
    assert abs(tv - uv) <= 1e-12 * uv and float(((tg - ug).abs() / ug).max()) <= 1e-12
    value, grad = WU.plain_fp32(p, y, st, [1.0] * 4)
    plain = U.plain_fp32(p, y, st)
    assert value.tobytes() == plain[0].tobytes() and np.array_equal(grad.view(np.int32), plain[1].view(np.int32))


def test_every_planted_mutation_is_rejected():
    cases = {'swap_weights': ('ce+dice', 2, None), 'weight_missing_in_member': ('ce+focal+dice', 2, 0.25), 'weight_twice': ('focal+dice', 2, 0.25)}
    assert set(cases) == set(WU.MUTATIONS)
    for mut in WU.MUTATIONS:
        for terms, g, fa in (cases[mut], ('ce+focal+dice', 2, None)) + ((('dice', 2, None), ('ce', 2, None)) if mut != 'weight_missing_in_member' else ()):
            for N, HW, C in ((2, 7, 3), (3, 900, 4)):
                p, y = U.inputs(N, HW, C, _head(terms), 50 + HW)
                w = WU.weights_for(C)
                st = U.Settings(terms, g, fa, 1.0, alpha=200.0)
                want = WU.Expect(p, y, st, w)
                rv, rg = want.ratios(*WU.plain_fp32(p, y, st, w))
                assert rv <= 1.0 and rg <= 1.0
                mv, mg = want.ratios(*WU.plain_fp32(p, y, st, w, mutate=mut))
                print(f'{mut} on {terms} ({N},{HW},{C}): value {mv:.3g}, gradient {mg:.3g} of the bound')
                assert not mv <= 1.0 and not mg <= 1.0, (mut, terms, mv, mg)          # both the value and the gradient show it


# ---- the C ABI's argument checks (no launch is reached: these run without a device) -----------------------------------------------------------

def test_argument_errors_before_any_launch():
    from patchgan_amd import _lib as L
    lib = L.load()
    N, HW, C = 2, 4096, 4
    need = lib.pg_seg_loss_workspace_bytes(N, HW, C)
    P, Y, G, V, WS, CW, CNT = 4096, 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25      # (never dereferenced: every call below is refused)
    ok = dict(p=P, ld_p=8, y=Y, ld_y=8, N=N, HW=HW, C=C, terms=L.SEG_CE | L.SEG_DICE, gamma=2, fa=L.SEG_FOCAL_ALPHA_NONE, smooth=1.0,
              ws=WS, nb=need, g=G, ld_g=4, value=V, cw=CW)

    def finish(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_value_grad_w(a['ws'], a['nb'], a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'],
                                            a['fa'], a['smooth'], 0.1, 0.1, 0.1, a['cw'], a['g'], a['ld_g'], a['value'], None)
    bad = [dict(cw=None), dict(p=None), dict(y=None), dict(value=None), dict(ws=None), dict(ws=WS + 4), dict(nb=need - 8), dict(N=0), dict(HW=0),
           dict(C=0), dict(ld_p=3), dict(ld_y=3), dict(ld_g=3), dict(terms=0), dict(terms=8), dict(terms=L.SEG_CE, C=1, ld_p=1, ld_y=1),
           dict(gamma=-1), dict(gamma=9), dict(fa=0.0), dict(fa=1.0), dict(fa=float('nan')), dict(smooth=0.0), dict(smooth=float('inf')),
           dict(smooth=float('nan'))]
    for kw in bad:
        assert finish(**kw) == -1, kw

    def count(**kw):
        a = dict(dict(y=Y, ld_y=8, N=N, HW=HW, C=C, counts=CNT), **kw)
        return lib.pg_seg_label_count(a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['counts'], None)
    for kw in (dict(y=None), dict(counts=None), dict(N=0), dict(N=-1), dict(HW=0), dict(C=0), dict(C=-3), dict(ld_y=3), dict(C=40, ld_y=39)):
        assert count(**kw) == -1, kw


def test_class_weights_file_is_plain_json(tmp_path):
    """_class_weights_restore(): the file an estimate left is taken where the setting is the scheme it was made with, and only then."""
    t = _trainer(tmp_path)
    t.loss_type = 'ce+dice'
    info = {'scheme': 'balanced', 'counts': [2, 1, 1, 0], 'unlabelled': 3, 'pixels': 7, 'weights': [0.5, 1.0, 1.0, 1.5]}
    (tmp_path / 'class_weights.json').write_text(json.dumps(info))
    t.class_weights = 'balanced_sqrt'
    assert not t._class_weights_restore() and t.class_weights == 'balanced_sqrt'
    t.class_weights = None
    assert not t._class_weights_restore() and t.class_weights is None
    t.class_weights = [1, 2, 3, 4]
    assert not t._class_weights_restore() and t.class_weights == [1, 2, 3, 4]
    t.class_weights = 'balanced'
    assert t._class_weights_restore() and t.class_weights == [0.5, 1.0, 1.0, 1.5] and t.class_weight_info == info
    t.class_weights = 'balanced'
    t.load_last_checkpoint()          # (no checkpoint in the folder: the weights are restored all the same)
    assert t.class_weights == [0.5, 1.0, 1.0, 1.5]
    assert t._seg_now().class_weights == (0.5, 1.0, 1.0, 1.5)
