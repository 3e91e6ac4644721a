"""The GAN objectives without a GPU (Trainer.gan_mode / real_label, Discriminator(final_act=...), pg_gan_loss's argument checks): the
float64 references against torch's named functions and their autograd, the plain-fp32 evaluation against the bounds, the planted
mutations against the comparator, the oracle trainer's defaults against OracleTrainer, the validation errors and the YAML helpers."""
import ctypes

import numpy as np
import pytest
import torch
import yaml

from tests import ganloss_util as U
from tests.golden_util import Golden, LOSS_KEYS

SIZES = ((1, 1), (2, 7), (3, 900), (16, 900), (2, 15876))
TERMS = [(name, t) for name in U.KINDS for t in ((1.0, 0.0) if name == 'hinge_d' else (1.0, 0.0, 0.9) if name != 'hinge_g' else (1.0,))]


# ---- references, emulation, comparator -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,t', TERMS)
def test_references_equal_torch_autograd(name, t):
    kind = U.KINDS[name]
    for N, HW in SIZES[:4]:
        d, scale = U.patch_values(N * HW, N * 1000 + HW), U.scale_of(0.5, 2 * N, HW)
        v, g = U.term_ref(kind, d, t, scale)
        tv, tg = U.term_torch(kind, d, t, scale)
        assert abs(v - tv) <= 1e-13 * max(abs(tv), 1e-300), (N, HW, v, tv)
        assert np.abs(g - tg).max() <= 1e-13 * np.abs(tg).max(), (N, HW)
    # the planted margins: exactly on a margin the value and the gradient are 0, one fp32 step inside they are not (torch's relu backward)
    if name == 'hinge_d':
        m = 1.0 if t == 1.0 else -1.0
        inside = m * (1.0 - 2.0 ** -23)
        _, g = U.term_torch(kind, np.array([m, inside, m * (1.0 + 2.0 ** -23)]), t, 1.0)
        assert list(g) == [0.0, -m, 0.0]
        assert np.array_equal(U.term_ref(kind, np.array([m, inside, m * (1.0 + 2.0 ** -23)]), t, 1.0)[1], g)


@pytest.mark.parametrize('name,t', TERMS)
def test_fp32_emulation_stays_below_every_bound(name, t):
    kind = U.KINDS[name]
    for N, HW in SIZES:
        for alpha, ranks in ((1.0, 1), (0.5, 2)):
            d, scale = U.patch_values(N * HW, N * 1000 + HW), U.scale_of(alpha, ranks * N, HW)
            rv, rg = U.ratios(kind, d, t, scale, *U.term_fp32(kind, d, t, scale))
            assert rv < 1.0 and rg < 1.0, (N, HW, alpha, rv, rg)


def test_comparator_rejects_the_planted_mutations():
    N, HW = 3, 900
    d = U.patch_values(N * HW, 7)
    scale = U.scale_of(0.5, N, HW)
    bad = lambda kind, t, s=scale, tt=None, mut=None: max(U.ratios(kind, d, t, scale, *U.term_fp32(kind, d, t if tt is None else tt, s, mut)))
    for t in (1.0, 0.0):
        assert bad(U.HINGE_D, t) < 1.0
        assert bad(U.HINGE_D, t, mut='hinge_sign') == float('inf')
        # >= instead of >: only the planted d = +-1 can tell (the value does not change: the element is 0 either way)
        v, g = U.term_fp32(U.HINGE_D, d, t, scale, 'hinge_ge')
        good = U.term_fp32(U.HINGE_D, d, t, scale)[1]
        assert int((g != good).sum()) == 1 and U.ratios(U.HINGE_D, d, t, scale, v, g)[1] == float('inf')
    assert bad(U.HINGE_G, 1.0, mut='hinge_sign') == float('inf')
    assert bad(U.LSGAN, 1.0) < 1.0 and bad(U.LSGAN, 1.0, mut='lsgan_no2') > 1e5
    # the divisor: this rank's N * HW instead of the global batch's (two ranks)
    half = U.scale_of(0.5, 2 * N, HW)
    for kind in U.KINDS.values():
        rv, rg = U.ratios(kind, d, 1.0, half, *U.term_fp32(kind, d, 1.0, scale))
        assert rv > 1e5 and (rg > 1e5), (kind, rv, rg)
    # label smoothing applied to the generator's target
    for kind in (U.LSGAN, U.BCE_LOGITS):
        assert bad(kind, 1.0, tt=0.9) > 1e4
    # softplus as log(1 + exp(d)): d = 90 is planted
    assert 90.0 in d
    assert bad(U.BCE_LOGITS, 0.0) < 1.0
    assert not bad(U.BCE_LOGITS, 0.0, mut='naive_softplus') <= 1.0


def test_step_terms_never_smooth_the_generator():
    for mode in U.GAN_MODES:
        for fa in ('sigmoid', 'none'):
            terms = U.step_terms(mode, fa, 0.9 if mode != 'hinge' else 1.0)
            if mode == 'hinge' and fa == 'sigmoid':
                continue
            assert (terms is None) == (mode == 'vanilla' and fa == 'sigmoid')
            if terms is not None:
                assert terms['gen'][1:] == (1.0, 1.0) and terms['fake'][1:] == (0.0, 0.5) and terms['real'][2] == 0.5


# ---- the oracle trainer ------------------------------------------------------------------------------------------------------------------

def test_default_oracle_is_the_oracle_bit_for_bit():
    from oracle.patchgan_oracle import OracleTrainer
    gold = Golden('a_lrelu_tversky')
    c = gold.cfg
    x, y = gold.inputs()
    args = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=c['loss_type'])
    a, b = OracleTrainer(gold.weights('g0'), gold.weights('d0'), **args), U.gan_oracle(gold, torch.float32)
    la, lb = a.batch(x, y, train=True), b.batch(x, y, train=True)
    assert [la[k] for k in LOSS_KEYS] == [lb[k] for k in LOSS_KEYS]
    for wa, wb in ((a.gw, b.gw), (a.dw, b.dw)):
        assert all(torch.equal(wa[k], wb[k]) for k in wa)
    assert all(torch.equal(a.last[w][k], b.last[w][k]) for w in ('g_grads', 'd_grads') for k in a.last[w])


def test_oracle_objectives_are_the_definitions():
    """One evaluation step per mode: the reported terms are the float64 references of the patch maps the oracle saw."""
    gold = Golden('a_lrelu_tversky')
    x, y = gold.inputs()
    for mode, r, fa in (('lsgan', 0.9, 'none'), ('lsgan', 1.0, 'sigmoid'), ('vanilla', 0.9, 'none'), ('hinge', 1.0, 'none')):
        o = U.gan_oracle(gold, torch.float64, mode, r, fa, 256.0 if mode == 'hinge' else 1.0)
        l = o.batch(x, y, train=False)
        terms = U.step_terms(mode, fa, r)
        dr, df = o.last['d_real'].numpy().ravel(), o.last['d_fake'].numpy().ravel()
        for key, d, (kind, t, _alpha) in (('gdisc', df, terms['gen']), ('discr', dr, terms['real']), ('discf', df, terms['fake'])):
            # (the reference at the float64 target, not its fp32 rounding: elem_ref rounds t)
            want = U.term_torch(U.KINDS[kind], d, t, 1.0 / d.size)[0] if U.f32(t) == t else None
            if want is not None:
                assert abs(l[key] - want) <= 1e-12 * abs(want), (mode, key)
        assert abs(l['disc'] - (l['discr'] + l['discf']) / 2) <= 1e-15 * abs(l['disc'])


# ---- the module and the trainer's checks ---------------------------------------------------------------------------------------------------

def test_final_act_of_the_discriminator():
    import patchgan_amd as pg
    for bad in ('tanh', None, 0, 'Sigmoid', True):
        with pytest.raises(ValueError):
            pg.Discriminator(5, 8, final_act=bad)
    sds = {}
    for fa in ('sigmoid', 'none'):
        torch.manual_seed(11)
        d = pg.Discriminator(5, 8, final_act=fa)
        assert d.final_act == fa and d.engine.layers[-1].act == fa
        with pytest.raises(AttributeError):
            d.final_act = 'none'
        sds[fa] = d.state_dict()
        assert [l.act for l in d.engine.layers[:-1]] == ['leakyrelu', 'tanh', 'tanh', 'tanh']
    assert pg.Discriminator(5, 8).final_act == 'sigmoid'
    assert list(sds['sigmoid']) == list(sds['none'])
    assert all(torch.equal(sds['sigmoid'][k], sds['none'][k]) for k in sds['none'])
    a, b = pg.Discriminator(5, 8).engine.layers, pg.Discriminator(5, 8, final_act='none').engine.layers
    assert [(l.key, l.p_off, l.b_off) for l in a] == [(l.key, l.p_off, l.b_off) for l in b]


def _trainer(tmp_path, **dkw):
    import patchgan_amd as pg
    g = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3, **dkw)
    return pg.Trainer(g, d, str(tmp_path))


def test_trainer_validation_comes_before_any_launch(tmp_path):
    import patchgan_amd as pg
    assert pg.Trainer.gan_mode == 'vanilla' and pg.Trainer.real_label == 1.0
    x = torch.zeros(2, 3, 256, 256)
    cases = [('sigmoid', dict(gan_mode='wgan')), ('sigmoid', dict(gan_mode=None)), ('sigmoid', dict(gan_mode='hinge')),
             ('none', dict(gan_mode='hinge', real_label=0.9)), ('none', dict(gan_mode='lsgan', real_label=0.0)),
             ('sigmoid', dict(real_label=1.5)), ('sigmoid', dict(real_label=-0.1)), ('sigmoid', dict(real_label='1')),
             ('none', dict(gan_mode='lsgan', real_label=float('nan')))]
    for fa, attrs in cases:
        t = _trainer(tmp_path, final_act=fa)
        for k, v in attrs.items():
            setattr(t, k, v)
        with pytest.raises(ValueError):          # (CPU tensors: anything later than the check would raise RuntimeError instead)
            t.batch(x, x[:, :1], train=True)
        with pytest.raises(ValueError):
            t.batch(x, x[:, :1], train=False)
    for fa, attrs in (('none', dict(gan_mode='hinge')), ('none', dict(gan_mode='lsgan', real_label=0.9)), ('sigmoid', dict(gan_mode='lsgan')),
                      ('none', dict()), ('sigmoid', dict(real_label=0.9)), ('sigmoid', dict(real_label=1))):
        t = _trainer(tmp_path, final_act=fa)
        for k, v in attrs.items():
            setattr(t, k, v)
        assert t._gan_now() == (attrs.get('gan_mode', 'vanilla'), float(attrs.get('real_label', 1.0)), fa)
        with pytest.raises(RuntimeError):        # valid settings: the step gets as far as asking for a HIP device
            t.batch(x, x[:, :1], train=True)


def test_kind_key_gains_the_objective_only_when_it_is_not_the_default(tmp_path):
    x = torch.zeros(2, 3, 256, 256)
    args = (x, x[:, :1], False, (2, 256, 256, 3, 1))
    t = _trainer(tmp_path)
    t.setup_optimizers()
    off = t._kind_key(*args, True)
    t.gan_mode, t.real_label = 'vanilla', 1
    assert t._kind_key(*args, True) == off and t._gan_key() == ()
    keys = {off}
    for fa, mode, r in (('sigmoid', 'vanilla', 0.9), ('sigmoid', 'lsgan', 1.0), ('none', 'vanilla', 1.0), ('none', 'lsgan', 1.0),
                        ('none', 'lsgan', 0.9), ('none', 'hinge', 1.0)):
        t = _trainer(tmp_path, final_act=fa)
        t.setup_optimizers()
        t.gan_mode, t.real_label = mode, r
        for train in (True, False):
            k = t._kind_key(*args, train)
            assert k[-1] == (mode, r, fa) and k not in keys
            keys.add(k)


def test_losses_module_has_the_torch_versions():
    import patchgan
    from patchgan_amd import losses
    d = torch.tensor(U.patch_values(64, 3)[:60].astype(np.float64)).reshape(2, 1, 5, 6)
    dr, df = d, -d.flip(0)
    n = d.numel()
    ref = lambda kind, x, t: U.term_ref(kind, x.numpy().ravel(), t, 1.0 / n)[0]
    assert abs(float(losses.lsgan_loss(d, 1.0)) - ref(U.LSGAN, d, 1.0)) < 1e-9 * ref(U.LSGAN, d, 1.0)
    assert abs(float(losses.lsgan_loss(d, torch.zeros_like(d))) - ref(U.LSGAN, d, 0.0)) < 1e-9 * ref(U.LSGAN, d, 0.0)
    want = (ref(U.HINGE_D, dr, 1.0) + ref(U.HINGE_D, df, 0.0)) / 2
    assert abs(float(losses.hinge_d_loss(dr, df)) - want) < 1e-12 * want
    assert abs(float(losses.hinge_g_loss(df)) - ref(U.HINGE_G, df, 1.0)) < 1e-12 * abs(ref(U.HINGE_G, df, 1.0))
    import patchgan.losses
    assert patchgan.losses.hinge_g_loss is losses.hinge_g_loss and patchgan.losses.lsgan_loss is losses.lsgan_loss


# ---- the C ABI's argument checks (no launch is reached: these run without a device) ------------------------------------------------------

def test_argument_errors_before_any_launch():
    from patchgan_amd import _lib as L
    lib = L.load()
    assert lib.pg_gan_loss_max_terms() == L.GAN_MAX_TERMS >= 2 and ctypes.sizeof(L.GanTerm) == 56
    assert 14400 <= lib.pg_gan_loss_single_max() < 2 * 15876

    def items(count=2, **kw):
        it = (L.GanTerm * count)()
        for t in it:
            t.d, t.g, t.value, t.scale, t.n, t.ld, t.ld_g, t.kind, t.target = 4096, 8192, 12288, 0.5, 100, 1, 1, L.GAN_LSGAN, 1.0
        for k, v in kw.items():
            setattr(it[-1], k, v)
        return it
    bad = [items(d=None), items(value=None), items(n=0), items(n=-5), items(ld=0), items(ld_g=0), items(kind=4), items(kind=-1),
           items(kind=L.GAN_HINGE_D, target=0.9), items(kind=L.GAN_HINGE_D, target=float('nan'))]
    for it in bad:
        assert lib.pg_gan_loss(2, it, None, 0, None) == -1
        assert lib.pg_gan_loss_workspace_bytes(2, it) == 0
    assert lib.pg_gan_loss(0, items(), None, 0, None) == -1 and lib.pg_gan_loss(2, None, None, 0, None) == -1
    assert lib.pg_gan_loss(L.GAN_MAX_TERMS + 1, items(L.GAN_MAX_TERMS + 1), None, 0, None) == -1
    # a term beyond the one-launch path: the call needs its workspace
    big = items(n=lib.pg_gan_loss_single_max() + 1)
    need = lib.pg_gan_loss_workspace_bytes(2, big)
    assert need > 0 and need % 8 == 0 and lib.pg_gan_loss_workspace_bytes(2, items()) == 0
    assert lib.pg_gan_loss(2, big, None, need, None) == -1
    assert lib.pg_gan_loss(2, big, 4096, need - 8, None) == -1
    assert lib.pg_gan_loss(2, big, 4100, need, None) == -1


# ---- the YAML ------------------------------------------------------------------------------------------------------------------------------

NESTED = """
model_params:
  generator: {filters: 4, activation: leakyrelu}
  discriminator: {filters: 4, n_layers: 3%s}
"""
FLAT = """
model_params: {gen_filts: 4, disc_filts: 4, n_disc_layers: 3, activation: tanh%s}
"""
TRAIN_YAML = """
train_params:
  loss_type: weighted_bce
  seg_alpha: 200
%s
"""


def test_yaml_helpers_both_schemas(tmp_path):
    from patchgan_amd.train import apply_train_params, disc_final_act_of, gan_mode_of, model_cfgs
    assert disc_final_act_of() == 'sigmoid' and disc_final_act_of('none') == 'none'
    for text, want in ((NESTED % '', None), (NESTED % ', final_act: none', 'none'), (NESTED % ', final_act: sigmoid', 'sigmoid'),
                       (FLAT % '', None), (FLAT % ', disc_final_act: none', 'none')):
        assert model_cfgs(yaml.safe_load(text)['model_params'])[1].get('final_act') == want
    for text in (NESTED % ', final_act: tanh', NESTED % ', final_act: true', FLAT % ', disc_final_act: logits', FLAT % ', disc_final_act: 0'):
        with pytest.raises(ValueError):
            model_cfgs(yaml.safe_load(text)['model_params'])
    assert gan_mode_of() == ('vanilla', 1.0) and gan_mode_of('hinge', None, 'none') == ('hinge', 1.0)
    assert gan_mode_of('lsgan', 0.9) == ('lsgan', 0.9)
    for args in (('hinge',), ('hinge', 0.9, 'none'), ('wgan',), ('vanilla', 0), ('vanilla', 2), ('vanilla', 'x'), (3,)):
        with pytest.raises(ValueError):
            gan_mode_of(*args)
    t = _trainer(tmp_path, final_act='none')
    for text, mode, r in (('', 'vanilla', 1.0), ('  gan_mode: hinge', 'hinge', 1.0), ('  gan_mode: lsgan\n  real_label: 0.9', 'lsgan', 0.9),
                          ('  real_label: 0.8', 'vanilla', 0.8)):
        apply_train_params(t, yaml.safe_load(TRAIN_YAML % text)['train_params'])
        assert (t.gan_mode, t.real_label) == (mode, r) and t.loss_type == 'weighted_bce'
    for text in ('  gan_mode: wasserstein', '  gan_mode: hinge\n  real_label: 0.9', '  real_label: 0', '  gan_mode: [hinge]'):
        with pytest.raises(ValueError):
            apply_train_params(t, yaml.safe_load(TRAIN_YAML % text)['train_params'])
    with pytest.raises(ValueError):          # hinge against a sigmoid head
        apply_train_params(_trainer(tmp_path), yaml.safe_load(TRAIN_YAML % '  gan_mode: hinge')['train_params'])
