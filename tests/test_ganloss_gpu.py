"""The GAN objectives on the GPU (Trainer.gan_mode / real_label, Discriminator(final_act='none'); ganloss.hip): pg_gan_loss against the
float64 references between guards, the logit discriminator against float64 F.conv2d autograd, and the trainer -- one-step gradients, a
three-step curve, the launch modes, off-is-off, label smoothing, evaluation steps, data parallelism and the smoke checks -- against
GanOracleTrainer.  Needs an MI355X."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import ganloss_util as U
from tests import guard_util as GU
from tests.golden_util import Golden, LOSS_KEYS

pytestmark = pytest.mark.gpu

EINVAL = -1
SIZES = ((1, 1), (2, 7), (3, 900), (16, 900), (2, 15876))          # the last: the 126 x 126 map of a 1024^2 input, beyond the one-launch path
TERMS = [(name, t) for name in U.KINDS for t in ((1.0, 0.0) if name == 'hinge_d' else (1.0, 0.0, 0.9) if name != 'hinge_g' else (1.0,))]


def _L():
    from patchgan_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- A. the kernel
class _Term:
    """One term between guards: d in a view of pixel stride ld at channel offset off (the other channels stay poison), its gradient
    view of the same layout (or none) and the slot of a guarded value block."""

    def __init__(self, kind, d, N, HW, t, scale, ld=1, off=0, grad=True, views=None):
        self.kind, self.d, self.t, self.scale = kind, np.asarray(d, dtype=np.float32), t, scale
        if views is None:
            x = torch.from_numpy(self.d.reshape(N, 1, 1, HW))
            self.dv, self.dg = GU.view_from(x, ld, off)
            self.gv, self.gg = GU.view(N, 1, HW, 1, ld, off) if grad else (None, None)
        else:
            self.dv, self.dg, self.gv, self.gg = views

    def grad(self):
        v = self.gv
        return v.t[v.off:v.off + v.npix * v.ld:v.ld].cpu().numpy().copy()


def _call(terms, check=True):
    """One pg_gan_loss call over the terms; -> (values as np.float32 [n], the guarded value block, the workspace or None)."""
    L = _L()
    lib = L.load()
    items = (L.GanTerm * len(terms))()
    vals = GU.flat(4 * len(terms))
    for k, (it, t) in enumerate(zip(items, terms)):
        it.d, it.ld, it.n, it.kind, it.target, it.scale = t.dv.ptr(), t.dv.ld, t.dv.npix, t.kind, t.t, t.scale
        it.g, it.ld_g = (t.gv.ptr(), t.gv.ld) if t.gv is not None else (None, 0)
        it.value = vals.ptr() + 4 * k
    need = lib.pg_gan_loss_workspace_bytes(len(terms), items)
    big = any(t.dv.npix > lib.pg_gan_loss_single_max() for t in terms)
    assert (need > 0) == big
    ws = GU.flat(need) if need else None
    assert lib.pg_gan_loss(len(terms), items, ws.ptr() if ws else None, need, _stream()) == 0
    torch.cuda.synchronize()
    if check:
        GU.assert_untouched(vals, 'all', 'values')
        if ws is not None:
            GU.assert_untouched(ws, 'all', 'workspace')
        for t in terms:
            if t.gg is not None:
                GU.assert_untouched(t.gg, 'slice' if t.gg.kind == 'view' else 'all', 'gradient')
    return vals.inner(torch.float32).cpu().numpy().copy(), vals, ws


def _check(term, value, what):
    rv, rg = U.ratios(term.kind, term.d, term.t, term.scale, value, term.grad() if term.gv is not None else None)
    print(f'pg_gan_loss {what}: value {rv:.3f}, gradient {rg:.3f} of the bound')
    assert rv <= 1.0 and rg <= 1.0, (what, rv, rg)


@pytest.mark.parametrize('N,HW', SIZES)
@pytest.mark.parametrize('name,t', TERMS)
def test_kernel_against_float64(name, t, N, HW):
    kind = U.KINDS[name]
    d = U.patch_values(N * HW, N * 1000 + HW)
    ins = GU.Inputs()
    for ld, off in ((1, 0), (3, 1)):
        for alpha, ranks in ((1.0, 1), (0.5, 2)):
            scale = U.scale_of(alpha, ranks * N, HW)
            term = _Term(kind, d, N, HW, t, scale, ld, off)
            ins.add(term.dg, 'd')
            vals, _, _ = _call([term])
            _check(term, vals[0], f'{name} t={t} ({N},{HW}) ld={ld} alpha={alpha}')
            # value only: the same value bits, no gradient buffer to touch
            only = _Term(kind, d, N, HW, t, scale, ld, off, grad=False)
            assert _call([only])[0].view(np.int32)[0] == vals.view(np.int32)[0]
            # a second call: the same bits
            g1 = term.grad()
            again, _, _ = _call([term])
            assert again.view(np.int32)[0] == vals.view(np.int32)[0] and np.array_equal(term.grad().view(np.int32), g1.view(np.int32))
    ins.check('pg_gan_loss')


@pytest.mark.parametrize('N,HW', SIZES[2:])
@pytest.mark.parametrize('name,r', [('lsgan', 0.9), ('hinge_d', 1.0), ('hinge_g', 1.0), ('bce_logits', 0.9)])
def test_two_halves_of_one_buffer_in_one_call(name, r, N, HW):
    """The discriminator step's call: the real and the fake half of one 2N map as two terms of one launch, each against its own
    reference, and each with the bits the term gets in a call of its own."""
    kind = U.KINDS[name]
    d = U.patch_values(2 * N * HW, 5 * N + HW)
    d[N * HW:] = d[N * HW:][::-1]          # (planted values in the fake half as well, at its end)
    scale = U.scale_of(0.5, N, HW)
    dv, dg = GU.view_from(torch.from_numpy(d.reshape(2 * N, 1, 1, HW)))
    gv, gg = GU.view(2 * N, 1, HW, 1)
    halves = [_Term(kind, d[h * N * HW:(h + 1) * N * HW], N, HW, t, scale, views=(dv.samples(h * N, N), None, gv.samples(h * N, N), None))
              for h, t in ((0, r), (1, 0.0 if name != 'hinge_g' else 1.0))]
    snap = dg.snapshot()
    vals, _, _ = _call(halves)
    GU.assert_untouched(gg, 'all', 'gradient of both halves')
    GU.assert_unchanged(dg, snap, 'd')
    for h, term in enumerate(halves):
        _check(term, vals[h], f'{name} half {h} of ({N},{HW})')
        alone = _Term(kind, term.d, N, HW, term.t, scale)
        v1, _, _ = _call([alone])
        assert v1.view(np.int32)[0] == vals.view(np.int32)[h] and np.array_equal(alone.grad().view(np.int32), term.grad().view(np.int32))


@pytest.mark.parametrize('N,HW', [(3, 900), (2, 15876)])
@pytest.mark.parametrize('name,t', [('lsgan', 1.0), ('hinge_d', 1.0), ('hinge_d', 0.0), ('hinge_g', 1.0), ('bce_logits', 0.0), ('bce_logits', 1.0)])
def test_a_nan_comes_out_as_a_nan(name, t, N, HW):
    kind = U.KINDS[name]
    d = U.patch_values(N * HW, 17)
    where = np.array([0, 63, N * HW // 2, N * HW - 1])
    clean = _Term(kind, d, N, HW, t, U.scale_of(1.0, N, HW))
    _call([clean])
    d = d.copy()
    d[where] = np.nan
    term = _Term(kind, d, N, HW, t, U.scale_of(1.0, N, HW))
    vals, _, _ = _call([term])
    g = term.grad()
    assert np.isnan(vals[0]) and np.isnan(g[where]).all()
    rest = np.ones(N * HW, dtype=bool)
    rest[where] = False
    assert np.isfinite(g[rest]).all() and np.array_equal(g[rest].view(np.int32), clean.grad()[rest].view(np.int32))


def test_argument_errors_write_nothing():
    L = _L()
    lib = L.load()
    N, HW = 2, 15876
    d = U.patch_values(N * HW, 1)
    term = _Term(U.LSGAN, d, N, HW, 1.0, 1.0)
    vals = GU.flat(8)
    snap = term.dg.snapshot()

    def items(count=2, **kw):
        it = (L.GanTerm * count)()
        for k, x in enumerate(it):
            x.d, x.ld, x.n, x.kind, x.target, x.scale = term.dv.ptr(), 1, 100, L.GAN_LSGAN, 1.0, 0.5
            x.g, x.ld_g, x.value = term.gv.ptr(), 1, vals.ptr() + 4 * (k % 2)
        for k, v in kw.items():
            setattr(it[-1], k, v)
        return it
    for it in (items(d=None), items(value=None), items(n=0), items(ld=0), items(ld_g=0), items(kind=4), items(kind=L.GAN_HINGE_D, target=0.5)):
        assert lib.pg_gan_loss(2, it, None, 0, _stream()) == EINVAL
    assert lib.pg_gan_loss(0, items(), None, 0, _stream()) == EINVAL and lib.pg_gan_loss(2, None, None, 0, _stream()) == EINVAL
    assert lib.pg_gan_loss(L.GAN_MAX_TERMS + 1, items(L.GAN_MAX_TERMS + 1), None, 0, _stream()) == EINVAL
    big = items(n=N * HW)
    need = lib.pg_gan_loss_workspace_bytes(2, big)
    ws = GU.flat(need)
    assert need > 0
    assert lib.pg_gan_loss(2, big, None, need, _stream()) == EINVAL
    assert lib.pg_gan_loss(2, big, ws.ptr(), need - 8, _stream()) == EINVAL
    assert lib.pg_gan_loss(2, big, ws.ptr() + 4, need, _stream()) == EINVAL
    torch.cuda.synchronize()
    for g, what in ((vals, 'values'), (ws, 'workspace'), (term.gg, 'gradient')):
        GU.assert_untouched(g, None, what)
    GU.assert_unchanged(term.dg, snap, 'd')


# ---------------------------------------------------------------------------------------------- B. the module
def _rel(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _ref_disc(sd, x, gout, dtype, final_act):
    """(out, dx, {key: dparam}) of the oracle's discriminator on the weights sd, by autograd in `dtype`."""
    o = U.GanOracleTrainer({}, {k: v.detach().cpu() for k, v in sd.items()}, n_layers=3, norm=False, dtype=dtype)
    o.d_final_act = final_act
    xx = x.to(dtype).requires_grad_(True)
    out = o.D(xx)
    grads = torch.autograd.grad((out * gout.to(dtype)).sum(), [xx] + [o.dw[k] for k in o.dw])
    return out.detach(), grads[0], dict(zip(o.dw, grads[1:]))


def _module_cases():
    import patchgan_amd as pg
    torch.manual_seed(23)
    fresh = {fa: pg.Discriminator(5, 8, final_act=fa) for fa in ('none', 'sigmoid')}
    fresh['sigmoid'].load_state_dict(fresh['none'].state_dict())
    gold = Golden('a_lrelu_tversky')
    c = gold.cfg
    fix = {fa: pg.Discriminator(c['in_nc'] + c['out_nc'], c['ndf'], n_layers=c['n_layers'], norm=c['norm'], final_act=fa) for fa in ('none', 'sigmoid')}
    for d in fix.values():
        d.load_state_dict(gold.weights('d0'))
    x, y = gold.inputs()
    big = torch.cat((x, y), 1)
    rnd = torch.rand(2, 5, 256, 256, generator=torch.Generator().manual_seed(5))
    return [('fresh', fresh, rnd), ('fixture', fix, big)]


@pytest.mark.parametrize('size', [32, 256])
def test_logit_discriminator_against_float64_autograd(size):
    """forward() and backward() -- the input's and every parameter's gradient -- of Discriminator(final_act='none') against float64
    F.conv2d autograd, in the metric and bound tests/test_configs_gpu.py holds the discriminator's gradients to: relative max-norm <=
    max(2e-4, 4 x the fp32 oracle's own distance).  The head conv carries PG_ACT_NONE here, so the planner may give it another kernel
    than the sigmoid head's.  And sigmoid(logits) against the sigmoid module on the same weights: both lie within that bound of
    float64, so within twice it of each other."""
    for name, nets, x in _module_cases():
        x = x[:, :, :size, :size].contiguous()
        d = nets['none'].cuda()
        xin = x.cuda().requires_grad_(True)
        out = d(xin)
        assert tuple(out.shape) == (2, 1, size // 8 - 2, size // 8 - 2)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(size))
        out.backward(gout.cuda())
        sd = {k: v for k, v in d.state_dict().items()}
        o64, dx64, dp64 = _ref_disc(sd, x, gout, torch.float64, 'none')
        o32, dx32, dp32 = _ref_disc(sd, x, gout, torch.float32, 'none')
        rows = [('out', out.detach(), o64, o32), ('dx', xin.grad, dx64, dx32)] + [(k, p.grad, dp64[k], dp32[k]) for k, p in d.named_parameters()]
        assert len(rows) == 2 + len(dp64)
        for what, got, want, emu in rows:
            e, noise = _rel(got, want), _rel(emu, want)
            print(f'logit D {name} {size}: {what:18s} error {e:.2e} fp32-oracle noise {noise:.2e}')
            assert e <= max(2e-4, 4 * noise), (name, size, what, e, noise)
        p = nets['sigmoid'].cuda()(x.cuda()).detach()
        p64, p32 = torch.sigmoid(o64), torch.sigmoid(o32)
        bound = max(2e-4, 4 * _rel(p32, p64))
        e_p, e_s, e = _rel(p, p64), _rel(torch.sigmoid(out.detach()), p64), _rel(torch.sigmoid(out.detach()), p)
        print(f'logit D {name} {size}: sigmoid module {e_p:.2e}, sigmoid(logits) {e_s:.2e} from float64; from each other {e:.2e}')
        assert e_p <= bound and e_s <= bound and e <= 2 * bound


# ---------------------------------------------------------------------------------------------- C. the trainer
HEAD_GAIN = 256.0          # hinge: the fixture's logits lie within +-0.05; times 256 both sides of both margins are populated
# name -> (gan_mode, real_label, D's final_act, head gain)
COMBOS = {'lsgan_none': ('lsgan', 1.0, 'none', 1.0), 'lsgan_sigmoid': ('lsgan', 1.0, 'sigmoid', 1.0),
          'vanilla_none': ('vanilla', 1.0, 'none', 1.0), 'hinge': ('hinge', 1.0, 'none', HEAD_GAIN),
          'vanilla_smooth': ('vanilla', 0.9, 'sigmoid', 1.0)}


def _nets(combo='hinge', gold=None, nf=None, ndf=None, **dkw):
    """a_lrelu_tversky's networks with the fixture's weights (the head conv's times the combination's gain) and the combination's head;
    another width or discriminator option: torch's initialisation."""
    import patchgan_amd as pg
    gold = gold or Golden('a_lrelu_tversky')
    c = gold.cfg
    fa, gain = (COMBOS[combo][2], COMBOS[combo][3]) if combo is not None else ('sigmoid', 1.0)
    g = pg.UNet(c['in_nc'], c['out_nc'], nf or c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], ndf or c['ndf'], n_layers=c['n_layers'], norm=dkw.pop('norm', c['norm']), final_act=fa, **dkw)
    if nf is None:
        g.load_state_dict(gold.weights('g0'))
    if ndf is None and not dkw:
        dw = gold.weights('d0')
        dw[U.head_key(dw)] = dw[U.head_key(dw)] * gain
        d.load_state_dict(dw)
    return g.cuda(), d.cuda()


def _trainer(g, d, folder, combo='hinge', mode=None, **attrs):
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(folder))
    if combo is not None:
        t.gan_mode, t.real_label = COMBOS[combo][:2]
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers(1e-3, 1e-3)
    if mode is not None:
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    g.train()
    d.train()
    return t


def _oracle(gold, dtype, combo, **kw):
    m, r, fa, gain = COMBOS[combo]
    return U.gan_oracle(gold, dtype, m, r, fa, gain, **kw)


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


# How far the float64 oracle's one-step gradients (MAE, seg_alpha = 0) lie from the float64 VANILLA oracle's on the same weights, in
# units of the largest per-parameter bound, computed on the CPU with the two oracles: the generator's whole gradient / the
# discriminator's.  lsgan_none 2866 / 41545, lsgan_sigmoid 486 / 444, hinge 785 / 632: the test asks for 10 of both.  vanilla_none:
# 5.6e-13 / 7.8e-13 -- BCE with logits IS nn.BCELoss of the sigmoid, the same function of the weights, so no gradient can tell them
# apart (the test asks for the gradient to BE the vanilla oracle's within the bound; that the step took pg_gan_loss is
# test_off_is_off_and_the_launch_counts' matter).  vanilla_smooth: 0 / 1939 -- the generator's target is never smoothed, so its
# gradient is the vanilla one exactly; the discriminator's is held to 10.
SEPARATED = {'lsgan_none': (True, True), 'lsgan_sigmoid': (True, True), 'vanilla_none': (False, False), 'hinge': (True, True),
             'vanilla_smooth': (False, True)}


@pytest.mark.parametrize('combo', list(COMBOS))
def test_one_step_gradients_against_the_float64_oracle(tmp_path, combo):
    """seg_alpha = 0 with the MAE loss: the generator's gradient arrives only through D and the objective.  Every parameter's gradient of
    both networks after one training step against GanOracleTrainer(float64): relative L2 < 2e-2 and <= 8 x noise + 1e-3, noise the fp32
    oracle's own distance (the bound of test_diffaug_gpu.py::test_generator_gradient_through_the_adjoint).  Where the objective differs
    from the vanilla one as a function (SEPARATED) the whole gradient lies at least 10 x the largest such bound from the float64 vanilla
    oracle's.  Measured on an MI355X: every parameter's gradient at most 1.3e-05 in relative L2 from its float64 oracle (0.013 of its bound), a
    network's whole gradient 1.4e-07 .. 1.1e-06; from the vanilla oracle,
    in units of the largest bound, generator / discriminator: lsgan_none 2862 / 41536, lsgan_sigmoid 487 / 444, hinge 780 / 633,
    vanilla_smooth 0.0004 / 1952, vanilla_none 0.0004 / 0.0008."""
    gold = Golden('a_lrelu_tversky')
    x, y = gold.inputs()
    g, d = _nets(combo, gold)
    t = _trainer(g, d, tmp_path, combo, loss_type='MAE', seg_alpha=0)
    t.batch(x, y, train=True)
    t.flush()
    got = {'g_grads': {k: v.grad.detach().cpu() for k, v in g.named_parameters()}, 'd_grads': {k: v.grad.detach().cpu() for k, v in d.named_parameters()}}
    refs = {}
    for name, dtype, c in (('o64', torch.float64, combo), ('o32', torch.float32, combo), ('plain64', torch.float64, None)):
        o = _oracle(gold, dtype, c, loss_type='MAE', seg_alpha=0) if c else U.gan_oracle(gold, dtype, head_gain=COMBOS[combo][3], loss_type='MAE', seg_alpha=0)
        o.batch(x, y, train=True)
        refs[name] = o.last
    if combo == 'hinge':
        dr, df = refs['o64']['d_real'], refs['o64']['d_fake']
        sides = [float((dr < 1).double().mean()), float((dr > 1).double().mean()), float((df > -1).double().mean()), float((df < -1).double().mean())]
        print('hinge: share of the real term below / above +1, of the fake term above / below -1:', sides)
        assert min(sides) >= 0.10, sides
    for which, sep in zip(('g_grads', 'd_grads'), SEPARATED[combo]):
        worst = 0.0
        assert set(got[which]) == set(refs['o64'][which])
        for k, want in refs['o64'][which].items():
            e, noise = _l2(got[which][k], want), _l2(refs['o32'][which][k], want)
            print(f'{combo} {which} {k:40s} error {e:.2e} fp32-oracle noise {noise:.2e}')
            assert e < 2e-2 and e <= 8 * noise + 1e-3, (k, e, noise)
            worst = max(worst, 8 * noise + 1e-3)
        flat = lambda d_: torch.cat([d_[k].double().reshape(-1) for k in refs['o64'][which]])
        far, near = _l2(flat(got[which]), flat(refs['plain64'][which])), _l2(flat(got[which]), flat(refs['o64'][which]))
        print(f'{combo} {which}: {near:.2e} from the float64 oracle, {far:.2e} from the float64 VANILLA oracle = {far / worst:.1f} x the largest bound')
        assert (far >= 10 * worst) if sep else (far <= worst), (which, far, worst)
    t.release()


# The distance of a run from GanOracleTrainer(float64) on the same run is ONE number, as in test_diffaug_gpu.py: the largest relative
# error among the 18 loss scalars (each relative to its own value, floor 1e-6) and the parameter tensors of both networks after the third
# step (relative max-norm).  GanOracleTrainer(float32)'s own distance, computed on the CPU, per combination (the largest term is a
# weight tensor every time; the losses alone are at 1e-07 .. 4e-06) -- the bound is 3 x that:
CURVE_NOISE = {'lsgan_none': 4.238e-04, 'lsgan_sigmoid': 2.272e-02, 'vanilla_none': 3.007e-04, 'hinge': 9.263e-04, 'vanilla_smooth': 4.880e-04}


def _curve_dist(curve, want, weights, want_w):
    e_l = float((np.abs(curve - want) / np.maximum(np.abs(want), 1e-6)).max())
    e_w = max(float((weights[k].double().cpu() - w.double()).abs().max() / w.double().abs().max()) for k, w in want_w.items())
    return e_l, e_w


@pytest.mark.parametrize('combo', list(COMBOS))
def test_three_step_curve_against_the_float64_oracle(tmp_path, combo):
    """Three training steps with the fixture's loss: the six losses of every step and the final weights of both networks.  Measured on an
    MI355X (distance; the losses alone): lsgan_none 3.9e-04 (1.8e-05), lsgan_sigmoid 9.7e-04 (5.8e-07), vanilla_none 7.0e-04 (4.3e-07),
    hinge 4.7e-04 (9.0e-05), vanilla_smooth 3.5e-04 (7.6e-07)."""
    gold = Golden('a_lrelu_tversky')
    x, y = gold.inputs()
    g, d = _nets(combo, gold)
    t = _trainer(g, d, tmp_path, combo, loss_type=gold.cfg['loss_type'])
    o64 = _oracle(gold, torch.float64, combo)
    curve, want = [], []
    for s in range(3):
        l, w = t.batch(x, y, train=True), o64.batch(x, y, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
        want.append([w[k] for k in LOSS_KEYS])
    t.flush()
    got_w = {**{'g.' + k: v for k, v in g.state_dict().items()}, **{'d.' + k: v for k, v in d.state_dict().items()}}
    want_w = {**{'g.' + k: v.detach() for k, v in o64.gw.items()}, **{'d.' + k: v.detach() for k, v in o64.dw.items()}}
    e_l, e_w = _curve_dist(np.array(curve), np.array(want), got_w, want_w)
    bound = 3 * CURVE_NOISE[combo]
    print(f'{combo} 3-step curve vs float64 oracle: losses {e_l:.3e}, weights {e_w:.3e}; distance {max(e_l, e_w):.3e}, bound {bound:.3e}')
    assert max(e_l, e_w) <= bound, (e_l, e_w)
    t.release()


STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3): three replays
_MODE_RUNS = {}


def _mode_run(tmp_path_factory, mode):
    if mode not in _MODE_RUNS:
        g, d = _nets('hinge')
        x, y = Golden('a_lrelu_tversky').inputs()
        t = _trainer(g, d, tmp_path_factory.mktemp('gan_mode'), 'hinge', mode)
        rows, modes = [], []
        for s in range(STEPS):
            l = t.batch(x, y, train=True)
            rows.append([float(l[k]) for k in LOSS_KEYS])
            modes.append(t.launch_mode)
        t.flush()
        torch.cuda.synchronize()
        _MODE_RUNS[mode] = dict(losses=np.array(rows), modes=modes, g=g.flat.cpu().numpy().copy(), d=d.flat.cpu().numpy().copy())
        t.release()
    return _MODE_RUNS[mode]


@pytest.mark.parametrize('mode', ['eager2', 'graph'])
def test_launch_modes_are_bit_identical(tmp_path_factory, mode):
    one, other = _mode_run(tmp_path_factory, 'eager1'), _mode_run(tmp_path_factory, mode)
    assert other['modes'][3:] == [mode] * (STEPS - 3) and one['modes'] == ['eager1'] * STEPS, (one['modes'], other['modes'])
    assert np.array_equal(one['losses'], other['losses']), one['losses'] - other['losses']
    assert np.array_equal(one['g'], other['g']) and np.array_equal(one['d'], other['d'])
    assert np.isfinite(one['losses']).all()


class _Recorder:
    """Stands in for the loaded library: records the name of every entry point reached, calls through."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith('pg_'):
            self.names.append(name)
        return fn


def _recorded(tmp_path, monkeypatch, tag, combo, nsteps=3, train=True, **attrs):
    L = _L()
    x, y = Golden('a_lrelu_tversky').inputs()
    g, d = _nets(combo)
    t = _trainer(g, d, tmp_path / tag, combo, **attrs)
    rec = _Recorder(L.load())
    monkeypatch.setattr(L, '_lib', rec)
    rows = [[float(l[k]) for k in LOSS_KEYS] for l in (t.batch(x, y, train=train) for _ in range(nsteps))]
    t.flush()
    torch.cuda.synchronize()
    monkeypatch.undo()
    out = (np.array(rows), g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy(), rec.names)
    t.release()
    return out


def test_off_is_off_and_the_launch_counts(tmp_path, monkeypatch):
    """A trainer whose attributes were never set and one with gan_mode = 'vanilla', real_label = 1.0: the same library calls, the same
    bits, never pg_gan_loss.  With lsgan (on the same sigmoid discriminator) pg_gan_loss is reached exactly twice per training step and
    pg_loss_reduce_parts once (the segmentation loss) instead of four times; everything else is the off trainer's sequence."""
    never = _recorded(tmp_path, monkeypatch, 'never', None)
    explicit = _recorded(tmp_path, monkeypatch, 'explicit', None, gan_mode='vanilla', real_label=1.0)
    lsgan = _recorded(tmp_path, monkeypatch, 'lsgan', 'lsgan_sigmoid')
    for a, b in zip(never[:3], explicit[:3]):
        assert np.array_equal(a, b)
    assert never[3] == explicit[3] and len(never[3]) > 100
    assert not any('gan_loss' in n for n in never[3])
    assert never[3].count('pg_loss_reduce_parts') == 4 * 3 and never[3].count('pg_loss_value_grad') == 4 * 3
    on = lsgan[3]
    assert on.count('pg_gan_loss') == 2 * 3 and on.count('pg_loss_reduce_parts') == 3 and on.count('pg_loss_value_grad') == 3
    assert on.count('pg_gan_loss_workspace_bytes') == 2 * 3
    # (a BCE term is three entry points: the size query of its scratch, the reduction, value + gradient)
    bce_term = ('pg_loss_reduce_doubles', 'pg_loss_reduce_parts', 'pg_loss_value_grad')
    assert all(never[3].count(n) == 4 * 3 and on.count(n) == 3 for n in bce_term)
    other = lambda names: [n for n in names if 'gan_loss' not in n and n not in bce_term]
    assert other(on) == other(never[3])
    assert not np.array_equal(lsgan[0], never[0])


def test_label_smoothing_moves_the_real_term_only(tmp_path, monkeypatch):
    """real_label = 0.9 on the default pair (BCE on the sigmoid map): at step 1 gdisc and discf keep the off run's bits, discr differs
    and is the oracle's (within the curve bound of the combination); the step makes the off run's library calls."""
    off = _recorded(tmp_path, monkeypatch, 'off', None, nsteps=1)
    on = _recorded(tmp_path, monkeypatch, 'on', 'vanilla_smooth', nsteps=1)
    k = {n: i for i, n in enumerate(LOSS_KEYS)}
    assert on[3] == off[3]
    assert on[0][0, k['gdisc']] == off[0][0, k['gdisc']] and on[0][0, k['discf']] == off[0][0, k['discf']]
    assert on[0][0, k['discr']] != off[0][0, k['discr']]
    gold = Golden('a_lrelu_tversky')
    want = _oracle(gold, torch.float64, 'vanilla_smooth').batch(*gold.inputs(), train=True)
    for key in LOSS_KEYS:
        e = abs(on[0][0, k[key]] - want[key]) / max(abs(want[key]), 1e-6)
        print(f'real_label 0.9: {key} {on[0][0, k[key]]:.8f} oracle {want[key]:.8f} rel {e:.2e}')
        assert e <= 3 * CURVE_NOISE['vanilla_smooth'], (key, e)


@pytest.mark.parametrize('combo', ['hinge', 'lsgan_sigmoid', 'vanilla_none'])
def test_evaluation_step_values_and_no_update(tmp_path, monkeypatch, combo):
    """train=False: the six values against the float64 oracle (within the combination's curve bound), the objective evaluated by
    pg_gan_loss without a gradient, no weight of either network changed."""
    gold = Golden('a_lrelu_tversky')
    g, d = _nets(combo, gold)
    g0, d0 = g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy()
    rows, g1, d1, names = _recorded(tmp_path, monkeypatch, 'eval', combo, nsteps=1, train=False)
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert names.count('pg_gan_loss') == 2 and not any(n.startswith('pg_adam') for n in names)
    want = _oracle(gold, torch.float64, combo).batch(*gold.inputs(), train=False)
    for i, key in enumerate(LOSS_KEYS):
        e = abs(rows[0, i] - want[key]) / max(abs(want[key]), 1e-6)
        print(f'{combo} evaluation step: {key} {rows[0, i]:.8f} oracle {want[key]:.8f} rel {e:.2e}')
        assert e <= 3 * CURVE_NOISE[combo], (key, e)


# ---------------------------------------------------------------------------------------------- D. data parallelism
def _dp_worker(rank, world, port, q, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    g, d = _nets('hinge')
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tempfile.mkdtemp(), 'hinge')
    xs, ys = shard_batch(x, y, rank, world)
    curve = []
    for s in range(nsteps):
        l = t.batch(xs, ys, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, np.array(curve), g.flat.cpu().numpy(), d.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_against_the_single_process(tmp_path):
    """hinge on two ranks (gloo, both on the one GPU), each with half of the batch, against the single process on the whole batch:
    the comparison and bound of tests/test_dp_gpu.py for the default step."""
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    nsteps = 3
    g, d = _nets('hinge')
    x, y = Golden('a_lrelu_tversky').inputs()
    assert x.shape[0] == 2
    t = _trainer(g, d, tmp_path, 'hinge')
    single = np.array([[l[k] for k in LOSS_KEYS] for l in (t.batch(x, y, train=True) for _ in range(nsteps))])
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
    (_, c0, g0, d0), (_, c1, g1, d1) = res
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert np.allclose(c0, c1, rtol=1e-6)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('hinge dp2 vs single process: max rel err per step', err.max(axis=1))
    assert err.max() < 1e-4, err


# ---------------------------------------------------------------------------------------------- E. smoke checks
def _smoke(t, x, y, nsteps=2):
    rows = [[float(l[k]) for k in LOSS_KEYS] for l in (t.batch(x, y, train=True) for _ in range(nsteps))]
    t.flush()
    torch.cuda.synchronize()
    assert np.isfinite(rows).all(), rows
    return np.array(rows)


def test_every_option_together_runs(tmp_path):
    torch.manual_seed(3)
    g, d = _nets('hinge', spectral_norm=True)
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, 'hinge', ema_decay=0.99, diffaug='flip,translation,cutout', diffaug_seed=8, clip_grad_norm=1.0, two_streams=True)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all() and torch.isfinite(t.ema_generator.flat).all()
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['gen']['skipped'] == 0 and stats['disc']['skipped'] == 0
    t.release()


def test_bf16_networks_run(tmp_path):
    torch.manual_seed(99)
    g, d = _nets('lsgan_none', nf=16, ndf=32)
    g.set_precision('bf16')
    d.set_precision('bf16')
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, 'lsgan_none')
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all()
    t.release()


def test_batchnorm_discriminator_runs(tmp_path):
    from torch import nn
    torch.manual_seed(3)
    g, d = _nets('hinge', norm=True, norm_layer=nn.BatchNorm2d)
    x, y = Golden('a_lrelu_tversky').inputs()
    t = _trainer(g, d, tmp_path, 'hinge', two_streams=True)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all()
    t.release()
