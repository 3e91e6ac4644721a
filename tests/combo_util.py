"""Trainer's opt-in features turned on TOGETHER, restated as ONE functional trainer in torch autograd on the CPU (ComboOracleTrainer), the
list of combined settings the tests run (CASES), the distances the comparisons use and the committed tables that go with them.  Pure CPU:
nothing here launches a kernel; the library's modules are only constructed (torch's seeded initialisation) and asked for their
state_dict().

The per-feature oracles (GanOracleTrainer, AugOracleTrainer, SegOracleTrainer, WeightedSegOracleTrainer) each restate batch() whole and
cannot be stacked; none knows spectral normalisation, clipping, AdamW, the weight average or accumulation.  ComboOracleTrainer.batch holds
every option as a branch that is inert at its default: with everything off it is OracleTrainer operation for operation, with one family
on it is that family's oracle operation for operation (tests/test_combo_cpu.py holds it to both, bit for bit).

Distances (tests/test_combo_gpu.py and tests/test_combo_cpu.py use the same functions):
  gradients  per parameter tensor, relative L2 of the closed gradient of the FIRST update (with `accumulate` the window's mean) from the
             float64 oracle's: e < 2e-2 and e <= 8 noise + 1e-3, noise the float32 oracle's own distance for that parameter.
  curve      ONE number over three closed updates: the largest relative error among all loss scalars of all calls (each relative to its
             own value, floor 1e-6) and, after the last update, every parameter tensor of both networks, the weight average and u / v
             (each by relative max-norm).  Bound: 3 x COMBO_NOISE[case]['curve'], the float32 oracle's own distance.
A mutation counts as SEPARATED by a case when the float64 mutated oracle lies at least 10 x the case's largest bound from the float64 true
oracle, in the gradients (a network's whole gradient against the largest per-parameter bound) or in the curve."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.patchgan_oracle import adam_update, apply_act, bce, disc_plan, instance_norm, seg_loss, unet_forward
from tests import diffaug_util as A
from tests.golden_util import Golden, LOSS_KEYS
from tests.segweight_util import seg_objective, weights_for

REFERENCE_LOSSES = ('tversky', 'weighted_bce', 'MAE')
SN_EPS = 1e-12          # torch.nn.utils.spectral_norm's eps
ALL_POLICY = 'flip,translation,cutout'
OPTIM_BETAS, OPTIM_DECAY = ((0.5, 0.999), (0.0, 0.9)), (1e-2, None)
EMA_DECAY = 0.99
REAL_LABEL = 0.9          # the lsgan cases carry one-sided label smoothing
LR = 1e-3

MUTATIONS = ('fake_other_row', 'no_adjoint', 'sigma_before_iteration', 'iterate_per_pass', 'map_once_at_close', 'clip_per_call',
             'decay_every_call', 'ema_every_call', 'mean_twice', 'weights_skip_dice', 'real_label_on_gen', 'stale_dfake')


def _pair(v):
    """A per-network setting: one value for both networks or a pair (generator, discriminator)."""
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _betas(b):
    if b is None:
        return ((0.9, 0.999), (0.9, 0.999))
    if isinstance(b[0], (tuple, list)):
        return (tuple(b[0]), tuple(b[1]))
    return (tuple(b), tuple(b))


class ComboOracleTrainer:
    """Trainer.batch with every opt-in feature, functional, in `dtype` on the CPU.  gsd / dsd: the state_dict()s of a patchgan_amd UNet
    and Discriminator (with spectral = True the discriminator's carries weight_orig / weight_u / weight_v per conv).  Settings are
    attributes named as Trainer's; `table` is the differentiable augmentation's parameter table of the NEXT call (None = off: the test
    teacher-forces it), `mutate` one modelled interaction error out of MUTATIONS.
    last = {g_grads, d_grads (the closed gradients of the last update, by state_dict key), d_real, d_fake, coef_g, coef_d, sigma}."""

    keys = LOSS_KEYS

    def __init__(self, gsd, dsd, activation='tanh', final_act='sigmoid', n_layers=3, norm=False, loss_type='tversky', seg_alpha=200,
                 gen_lr=LR, dsc_lr=LR, tversky_beta=0.75, tversky_gamma=0.75, dtype=torch.float32, gan_mode='vanilla', real_label=1.0,
                 d_final_act='sigmoid', spectral=False, focal_gamma=2, focal_alpha=None, dice_smooth=1.0, class_weights=None, betas=None,
                 weight_decay=None, clip_grad_norm=None, ema_decay=None, accumulate=None, mutate=None):
        assert mutate is None or mutate in MUTATIONS, mutate
        self.dtype, self.mutate = dtype, mutate
        self.activation, self.final_act, self.n_layers, self.norm = activation, final_act, n_layers, norm
        self.loss_type, self.seg_alpha, self.beta, self.gamma = loss_type, seg_alpha, tversky_beta, tversky_gamma
        self.gen_lr, self.dsc_lr = gen_lr, dsc_lr
        self.gan_mode, self.real_label, self.d_final_act, self.spectral = gan_mode, real_label, d_final_act, spectral
        self.focal_gamma, self.focal_alpha, self.dice_smooth, self.class_weights = focal_gamma, focal_alpha, dice_smooth, class_weights
        self.betas, self.weight_decay, self.clip_grad_norm, self.ema_decay, self.accumulate = betas, weight_decay, clip_grad_norm, ema_decay, accumulate
        self.table = None
        par = lambda v: v.detach().clone().to(dtype).requires_grad_(True)
        self.gw = {k: par(v) for k, v in gsd.items()}
        # the discriminator's parameters under their state_dict keys (weight_orig with spectral normalisation); u, v are no parameters
        self.dw = {k: par(v) for k, v in dsd.items() if not k.endswith(('weight_u', 'weight_v'))}
        self.su = {k[:-len('.weight_u')]: v.detach().clone().to(dtype) for k, v in dsd.items() if k.endswith('weight_u')}
        self.sv = {k[:-len('.weight_v')]: v.detach().clone().to(dtype) for k, v in dsd.items() if k.endswith('weight_v')}
        assert bool(self.su) == bool(spectral) and len(self.su) == len(self.sv)
        self.wkey = 'weight_orig' if spectral else 'weight'
        zeros = lambda w: {k: torch.zeros_like(v) for k, v in w.items()}
        self.gm, self.gv, self.dm, self.dv = zeros(self.gw), zeros(self.gw), zeros(self.dw), zeros(self.dw)
        self.t_g = self.t_d = 0
        self.ema = {k: v.detach().clone() for k, v in self.gw.items()} if ema_decay is not None else None
        self.acc = {'g': None, 'd': None}
        self.acc_done = 0
        self.last = {}

    # ---- the networks
    def G(self, x):
        return unet_forward(self.gw, x, self.activation, self.final_act)

    def D(self, x, W):
        """disc_forward on the conv weights W ({state_dict stem: tensor}); the head's activation is d_final_act."""
        plan = disc_plan(x.shape[1], self.dw[f'model.0.{self.wkey}'].shape[0], self.n_layers, self.norm)
        h = x
        for li, (idx, _cin, _cout, stride, bias, act, has_norm) in enumerate(plan):
            b = self.dw[f'model.{idx}.bias'] if bias else None
            h = F.conv2d(h, W[f'model.{idx}'], b, stride=stride, padding=1)
            h = apply_act(h, act if li < len(plan) - 1 else self.d_final_act)
            if has_norm:
                h = instance_norm(h)
        return h

    def _stems(self):
        return [k[:-len('.' + self.wkey)] for k in self.dw if k.endswith('.' + self.wkey)]

    def _iterate(self):
        """One power iteration of every conv, as torch.nn.utils.spectral_norm's hook does it: u, v are constants of the graph."""
        with torch.no_grad():
            for s in self._stems():
                Wm = self.dw[f'{s}.weight_orig'].reshape(self.su[s].numel(), -1)
                self.sv[s] = F.normalize(torch.mv(Wm.t(), self.su[s]), dim=0, eps=SN_EPS)
                self.su[s] = F.normalize(torch.mv(Wm, self.sv[s]), dim=0, eps=SN_EPS)

    def _normalised(self, su=None, sv=None):
        """{stem: W / sigma} with sigma = u . (W v), differentiable to weight_orig; without spectral normalisation the weights."""
        if not self.spectral:
            return {s: self.dw[f'{s}.weight'] for s in self._stems()}, {}
        su, sv = su or self.su, sv or self.sv
        W, sig = {}, {}
        for s in self._stems():
            w = self.dw[f'{s}.weight_orig']
            sigma = torch.dot(su[s], torch.mv(w.reshape(su[s].numel(), -1), sv[s]))
            W[s], sig[s] = w / sigma, float(sigma.detach())
        return W, sig

    def _T(self, z, fake=False, straight=False):
        """The augmentation in front of a D call: real and fake sample i under the same row."""
        if self.table is None:
            return z
        table = np.asarray(self.table)
        if fake and self.mutate == 'fake_other_row':
            table = np.roll(table, 1, axis=0)
        t = A.apply_torch(z, table)
        if straight:          # 'no_adjoint': the value of T(z), the gradient of T's INPUT taken as it arrives at T's output
            return z + (t - z).detach()
        return t

    # ---- the objectives
    def _seg(self, gen_img, y):
        if self.loss_type in REFERENCE_LOSSES:
            return seg_loss(self.loss_type, gen_img, y, self.seg_alpha, self.beta, self.gamma)
        args = (self.seg_alpha, self.focal_gamma, self.focal_alpha, self.dice_smooth)
        members = self.loss_type.split('+')
        if self.mutate == 'weights_skip_dice' and len(members) > 1 and self.class_weights is not None:
            return (seg_objective(members[0], gen_img, y, *args, self.class_weights)
                    + seg_objective('+'.join(members[1:]), gen_img, y, *args, None))
        return seg_objective(self.loss_type, gen_img, y, *args, self.class_weights)

    def _gdisc(self, d_fake):
        if self.gan_mode == 'hinge':
            return -torch.mean(d_fake)
        r = self.real_label if self.mutate == 'real_label_on_gen' else 1.0          # (the generator's target is never smoothed)
        ones = torch.ones_like(d_fake) if r == 1.0 else torch.full_like(d_fake, r)
        if self.gan_mode == 'lsgan':
            return F.mse_loss(d_fake, ones)
        if self.d_final_act == 'none':
            return F.binary_cross_entropy_with_logits(d_fake, ones)
        return bce(d_fake, ones)

    def _real_fake(self, d_real, d_fake):
        r = self.real_label
        ones = torch.ones_like(d_real) if r == 1.0 else torch.full_like(d_real, r)
        zeros = torch.zeros_like(d_fake)
        if self.gan_mode == 'hinge':
            return torch.mean(F.relu(1.0 - d_real)), torch.mean(F.relu(1.0 + d_fake))
        if self.gan_mode == 'lsgan':
            return F.mse_loss(d_real, ones), F.mse_loss(d_fake, zeros)
        if self.d_final_act == 'none':
            return F.binary_cross_entropy_with_logits(d_real, ones), F.binary_cross_entropy_with_logits(d_fake, zeros)
        return bce(d_real, ones), bce(d_fake, zeros)

    # ---- the optimizer
    def _clip(self, grads, max_norm):
        """(grads * coef, coef) with coef = min(1, max_norm / (norm + 1e-6)) on the 2-norm of the whole gradient; (None, nan) where the
        norm is not finite: the update is skipped."""
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
        if not math.isfinite(norm):
            return None, float('nan')
        coef = min(1.0, max_norm / (norm + 1e-6))
        return {k: g * coef for k, g in grads.items()}, coef

    def _ema_step(self):
        with torch.no_grad():
            for k, w in self.gw.items():
                self.ema[k] += (w - self.ema[k]) * (1 - self.ema_decay)

    def _update(self, which, grads, phase, remap=None):
        """Network `which`'s gradient joins its window (phase None = accumulation off | 'open' | 'close') and, on a closing phase, the
        update runs once on the mean: clip, decay, Adam, the average; the step count advances once, skipped update or not."""
        i = 0 if which == 'g' else 1
        w, m, v = (self.gw, self.gm, self.gv) if i == 0 else (self.dw, self.dm, self.dv)
        lr, (b1, b2) = (self.gen_lr, self.dsc_lr)[i], _betas(self.betas)[i]
        wd = _pair(self.weight_decay)[i] if self.weight_decay is not None else None
        max_norm = _pair(self.clip_grad_norm)[i] if self.clip_grad_norm is not None else None
        mut = self.mutate
        if phase is not None:
            k = self.accumulate
            if mut == 'clip_per_call' and max_norm is not None:
                grads, coef = self._clip(grads, max_norm)
                self.last['coef_' + which] = coef
                max_norm = None
                if grads is None:
                    grads = {kk: torch.full_like(p, float('nan')) for kk, p in w.items()}
            acc = self.acc[which]
            total = grads if acc is None else {kk: acc[kk] + g for kk, g in grads.items()}
            if phase == 'open':
                self.acc[which] = total
                with torch.no_grad():
                    if mut == 'decay_every_call' and wd is not None:
                        for p in w.values():
                            p.mul_(1 - lr * wd)
                if mut == 'ema_every_call' and i == 0 and self.ema is not None:
                    self._ema_step()
                return
            self.acc[which] = None
            grads = {kk: g * (1.0 / k) for kk, g in total.items()}
            if mut == 'mean_twice':
                grads = {kk: g * (1.0 / k) for kk, g in grads.items()}
            if remap is not None:
                grads = remap(grads)
        self.last[which + '_grads'] = grads
        if i == 0:
            self.t_g += 1
        else:
            self.t_d += 1
        t = (self.t_g, self.t_d)[i]
        if max_norm is not None:
            grads, coef = self._clip(grads, max_norm)
            self.last['coef_' + which] = coef
            if grads is None:
                return          # a non-finite norm: weights, moments and the average keep their bits
        with torch.no_grad():
            for kk, g in grads.items():
                if wd is not None:
                    w[kk].mul_(1 - lr * wd)
                adam_update(w[kk], g, m[kk], v[kk], t, lr, b1, b2)
        if i == 0 and self.ema is not None:
            self._ema_step()

    # ---- one call
    def batch(self, x, y, train=False):
        x, y = x.to(self.dtype), y.to(self.dtype)
        mut = self.mutate
        phase = None
        if train and self.accumulate is not None and self.accumulate > 1:
            phase = 'close' if self.acc_done + 1 == self.accumulate else 'open'
            self.acc_done = 0 if phase == 'close' else self.acc_done + 1
        # spectral normalisation: one power iteration per training call, ahead of the first D pass; all three passes read that W / sigma
        if self.spectral:
            before = (dict(self.su), dict(self.sv))
            if train:
                self._iterate()
            W0, sigma = self._normalised(*before) if (mut == 'sigma_before_iteration' and train) else self._normalised()
            W1 = W2 = W0
            if mut == 'iterate_per_pass' and train:          # torch's per-forward semantics: each pass after an iteration of its own
                self._iterate()
                W1, _ = self._normalised()
                self._iterate()
                W2, _ = self._normalised()
            self.last['sigma'] = sigma
        else:
            W0 = W1 = W2 = self._normalised()[0]
        names_d = list(self.dw)

        gen_img = self.G(x)
        disc_fake = self.D(self._T(torch.cat((x, gen_img), 1), fake=True, straight=(mut == 'no_adjoint')), W0)
        gen_loss_seg = self._seg(gen_img, y)
        gen_loss_disc = self._gdisc(disc_fake)
        gen_loss = gen_loss_seg + gen_loss_disc
        if train:
            names = list(self.gw)
            grads = torch.autograd.grad(gen_loss, [self.gw[k] for k in names])
            self._update('g', dict(zip(names, grads)), phase)
        gen_fake = gen_img.detach()
        if mut == 'stale_dfake' and train:
            with torch.no_grad():
                gen_fake = self.G(x)          # the POST-update generator's output
        disc_real = self.D(self._T(torch.cat((x, y), 1)), W1)
        disc_fake2 = self.D(self._T(torch.cat((x, gen_fake), 1), fake=True), W2)
        self.last['d_real'], self.last['d_fake'] = disc_real.detach(), disc_fake2.detach()
        loss_real, loss_fake = self._real_fake(disc_real, disc_fake2)
        disc_loss = (loss_fake + loss_real) / 2.
        if train:
            if mut == 'map_once_at_close' and self.spectral and phase is not None:
                # the gradient of the NORMALISED weights joins the window; the closing call maps the mean through its own sigma, u, v
                stems = self._stems()
                leaves = [W0[s] if k.endswith('.weight_orig') else self.dw[k] for k, s in ((k, k[:-len('.weight_orig')]) for k in names_d)]
                raw = dict(zip(names_d, torch.autograd.grad(disc_loss, leaves, retain_graph=True)))

                def remap(mean):
                    mapped = torch.autograd.grad([W0[s] for s in stems], [self.dw[f'{s}.weight_orig'] for s in stems],
                                                 grad_outputs=[mean[f'{s}.weight_orig'] for s in stems])
                    out = dict(mean)
                    out.update({f'{s}.weight_orig': g for s, g in zip(stems, mapped)})
                    return out
                self._update('d', raw, phase, remap if phase == 'close' else None)
            else:
                grads = torch.autograd.grad(disc_loss, [self.dw[k] for k in names_d])
                self._update('d', dict(zip(names_d, grads)), phase)
        self.last['gen_img'] = gen_img.detach()
        vals = [gen_loss.item(), gen_loss.item(), gen_loss_disc.item(), loss_real.item(), loss_fake.item(), disc_loss.item()]
        return dict(zip(self.keys, vals))

    def step_accumulated(self):
        raise NotImplementedError('the oracle closes full windows only')

    def state(self):
        """Everything the curve distance looks at after the last update, by name."""
        out = {**{'g.' + k: v.detach() for k, v in self.gw.items()}, **{'d.' + k: v.detach() for k, v in self.dw.items()}}
        if self.ema is not None:
            out.update({'ema.' + k: v for k, v in self.ema.items()})
        out.update({f'd.{s}.weight_u': v for s, v in self.su.items()})
        out.update({f'd.{s}.weight_v': v for s, v in self.sv.items()})
        return out


# ---------------------------------------------------------------------------------------------------------------------- the cases
# Factors and levels (the first level of each is Trainer's default).  A case names a golden fixture for its SHAPES (channels, widths,
# depth, activations, batch, extent -- and the fixture's inputs for its first call); its modules are drawn by torch.manual_seed(seed).
FACTORS = {'gan': ('vanilla', 'lsgan', 'hinge'), 'spectral': (False, True), 'diffaug': (False, True), 'seg': ('ref', 'focal+dice', 'ce+dice'),
           'dnorm': (False, True), 'accumulate': (False, True), 'clip': (False, True), 'optim': (False, True), 'ema': (False, True)}
# what Trainer refuses: 'ce' needs the softmax head, which only d_softmax_tversky has, and 'focal+dice on a sigmoid head' excludes it --
# no pair of levels of two DIFFERENT factors is excluded by that (the fixture is not a factor); hinge on a sigmoid head is not a level.
REFUSED = ()

# gan level -> (gan_mode, the discriminator's final_act, real_label)
GAN_LEVELS = {'vanilla': ('vanilla', 'sigmoid', 1.0), 'lsgan': ('lsgan', 'none', REAL_LABEL), 'hinge': ('hinge', 'none', 1.0)}


def _case(fixture, seed, gan, spectral, diffaug, seg, dnorm, accumulate, clip, optim, ema, head_gain=1.0, aug_seed=0, lr=(LR, LR)):
    return dict(lr=lr, fixture=fixture, seed=seed, gan=gan, spectral=spectral, diffaug=diffaug, seg=seg, dnorm=dnorm, accumulate=accumulate,
                clip=clip, optim=optim, ema=ema, head_gain=head_gain, aug_seed=aug_seed)


A_, B_, D_ = 'a_lrelu_tversky', 'b_tanh_wbce_norm', 'd_softmax_tversky'
# clip: (generator max-norm, discriminator max-norm), each about half of the float64 oracle's first closed gradient norm -- except in
# `everything`, whose max-norms of 1e-8 put every element of the clipped gradient below Adam's eps: the update is then lr g / eps, linear
# in the gradient, the float32 oracle's weights stay within rounding of the float64 ones (no element takes its first steps with the other
# sign) and the curve's bound falls from ~1e-3 to ~1e-5.  Only there can the statistic see an error of lr x decay per call
# (decay_every_call; the generator's lr = 5e-2 makes that 5e-4) or of 0.01 |w - ema| per call (ema_every_call).
# lr: (generator, discriminator), 1e-3 unless given.
CASES = {
    #                      fixture seed gan        spectral diffaug seg           dnorm  accum  clip            optim  ema
    'everything':    _case(D_, 115, 'hinge',   True,  True,  'ce+dice',    True,  2,     (1e-8, 1e-8),   True,  True, lr=(5e-2, 1e-3)),
    'plain':         _case(A_, 102, 'vanilla', False, False, 'ref',        False, None,  None,           False, False),
    'hinge_shared':  _case(A_, 113, 'hinge',   False, True,  'focal+dice', False, None,  (1.5, 8.0),     True,  False, head_gain=256.0, aug_seed=3),
    'hinge_sn_ref':  _case(B_, 104, 'hinge',   True,  False, 'ref',        True,  3,     None,           False, False),
    'lsgan_sn':      _case(B_, 105, 'lsgan',   True,  True,  'focal+dice', False, 2,     None,           False, True, aug_seed=5),
    'lsgan_ce':      _case(D_, 106, 'lsgan',   False, False, 'ce+dice',    False, None,  (1000.0, 0.5),  False, False),
    'lsgan_ref':     _case(A_, 107, 'lsgan',   False, True,  'ref',        True,  None,  (10.0, 1.2),    True,  True, aug_seed=7),
    'vanilla_sn':    _case(B_, 108, 'vanilla', True,  False, 'focal+dice', True,  None,  (50.0, 0.5),    True,  True),
    'vanilla_ce':    _case(D_, 109, 'vanilla', True,  False, 'ce+dice',    False, 2,     None,           True,  True),
    'vanilla_accum': _case(A_, 110, 'vanilla', False, True,  'ref',        False, 2,     (10.0, 0.03),   False, True, aug_seed=10),
}
EVERYTHING = 'everything'


def levels_of(case):
    """The level of each factor a case sits on."""
    return {'gan': case['gan'], 'spectral': case['spectral'], 'diffaug': case['diffaug'], 'seg': case['seg'], 'dnorm': case['dnorm'],
            'accumulate': case['accumulate'] is not None, 'clip': case['clip'] is not None, 'optim': case['optim'], 'ema': case['ema']}


def missing_pairs(cases=None):
    """Every pair of levels of two different factors that no case holds together (and Trainer does not refuse)."""
    cases = CASES if cases is None else cases
    seen = set()
    for c in cases.values():
        lv = levels_of(c)
        seen.update(((f1, lv[f1]), (f2, lv[f2])) for f1 in FACTORS for f2 in FACTORS if f1 < f2)
    want = [((f1, a), (f2, b)) for f1 in FACTORS for f2 in FACTORS if f1 < f2 for a in FACTORS[f1] for b in FACTORS[f2]]
    return [p for p in want if p not in seen and p not in REFUSED]


def calls_of(case, updates=3):
    return updates * (case['accumulate'] or 1)


def loss_type_of(case, cfg):
    return cfg['loss_type'] if case['seg'] == 'ref' else case['seg']


def class_weights_of(case, cfg):
    return None if case['seg'] == 'ref' else weights_for(cfg['out_nc'])


def modules(name, **dkw):
    """(UNet, Discriminator) of a case on the CPU, drawn under torch.manual_seed(case seed), the head conv's weight times the case's
    gain; dkw: other constructor arguments of the discriminator (the launch-mode variants: norm_layer), use_dropout for the generator
    and nf / ndf for other widths than the fixture's."""
    import patchgan_amd as pg
    case = CASES[name]
    c = Golden(case['fixture']).cfg
    torch.manual_seed(case['seed'])
    g = pg.UNet(c['in_nc'], c['out_nc'], dkw.pop('nf', c['nf']), use_dropout=dkw.pop('use_dropout', False), activation=c['activation'],
                final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], dkw.pop('ndf', c['ndf']), n_layers=c['n_layers'], norm=case['dnorm'], spectral_norm=case['spectral'],
                         final_act=GAN_LEVELS[case['gan']][1], **dkw)
    if case['head_gain'] != 1.0:
        sd = d.state_dict()
        key = max((k for k in sd if k.endswith(('.weight', '.weight_orig'))), key=lambda k: int(k.split('.')[1]))
        sd[key] = sd[key] * case['head_gain']
        d.load_state_dict(sd)
    return g, d


def inputs(name, call):
    """(x, y) of call number `call` of a case: the fixture's own inputs first, then the same recipe under other seeds (the micro-batches
    of a window differ)."""
    gold = Golden(CASES[name]['fixture'])
    if call == 0:
        return gold.inputs()
    c = gold.cfg
    gen = torch.Generator().manual_seed(gold.data_seed + 1000 * call)
    x = torch.rand(c['B'], c['in_nc'], c['size'], c['size'], generator=gen)
    y = (torch.rand(c['B'], c['out_nc'], c['size'], c['size'], generator=gen) > 0.7).float()
    return x, y


def table(name, call):
    """The augmentation table of training call `call` (0-based) of a case, None with diffaug off: what pg_diffaug_params draws
    (tests/diffaug_util.params_ref; the GPU tests read the device's own table and hold it to this one)."""
    case = CASES[name]
    if not case['diffaug']:
        return None
    c = Golden(case['fixture']).cfg
    return A.params_ref(case['aug_seed'], call, 7, 0, c['B'], c['size'], c['size'])


def shares_dfake(name):
    """Whether the case's step takes the shared D(fake) pass: the planner's predicate for the case's discriminator and batch (both halves
    of a 256 x 256 fp32 buffer sit on one 16-byte phase)."""
    from patchgan_amd import engine as E
    case = CASES[name]
    c = Golden(case['fixture']).cfg
    de = E.DiscriminatorEngine(c['in_nc'] + c['out_nc'], c['ndf'], c['n_layers'], case['dnorm'], spectral=case['spectral'],
                               final_act=GAN_LEVELS[case['gan']][1])
    return bool(de.halves_ok(c['B'], c['size'], c['size']))


def mutation_applies(mutation, name):
    """Whether a mutation changes anything in a case (the factors it lives on are on)."""
    case = CASES[name]
    acc = case['accumulate'] is not None
    return {'fake_other_row': case['diffaug'] and Golden(case['fixture']).cfg['B'] > 1, 'no_adjoint': case['diffaug'],
            'sigma_before_iteration': case['spectral'], 'iterate_per_pass': case['spectral'], 'map_once_at_close': case['spectral'] and acc,
            'clip_per_call': case['clip'] is not None and acc, 'decay_every_call': case['optim'] and acc, 'ema_every_call': case['ema'] and acc,
            'mean_twice': acc, 'weights_skip_dice': case['seg'] != 'ref', 'real_label_on_gen': case['gan'] == 'lsgan', 'stale_dfake': True}[mutation]


def trainer_settings(name):
    """The case as attributes of patchgan_amd.Trainer (and of ComboOracleTrainer, which names them alike)."""
    case = CASES[name]
    c = Golden(case['fixture']).cfg
    mode, _fa, r = GAN_LEVELS[case['gan']]
    s = dict(gan_mode=mode, real_label=r, loss_type=loss_type_of(case, c), class_weights=class_weights_of(case, c))
    if case['accumulate'] is not None:
        s['accumulate'] = case['accumulate']
    if case['clip'] is not None:
        s['clip_grad_norm'] = case['clip']
    if case['optim']:
        s.update(betas=OPTIM_BETAS, weight_decay=OPTIM_DECAY)
    if case['ema']:
        s['ema_decay'] = EMA_DECAY
    return s


def oracle(name, dtype, gsd=None, dsd=None, mutate=None, **over):
    """ComboOracleTrainer of a case on the state dicts given (default: the case's own seeded modules)."""
    case = CASES[name]
    c = Golden(case['fixture']).cfg
    if gsd is None:
        g, d = modules(name)
        gsd, dsd = g.state_dict(), d.state_dict()
    kw = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=case['dnorm'], dtype=dtype,
              d_final_act=GAN_LEVELS[case['gan']][1], spectral=case['spectral'], mutate=mutate)
    kw.update(trainer_settings(name), gen_lr=case['lr'][0], dsc_lr=case['lr'][1])
    kw.update(over)
    return ComboOracleTrainer({k: v.detach().cpu() for k, v in gsd.items()}, {k: v.detach().cpu() for k, v in dsd.items()}, **kw)


def run(name, dtype, mutate=None, updates=3, gsd=None, dsd=None):
    """The case through its oracle: dict(first = the `last` of the first closed update (gradients, coefficients, sigma, d_real, d_fake),
    losses [calls, 6], state = ComboOracleTrainer.state() after the last update)."""
    o = oracle(name, dtype, gsd, dsd, mutate)
    k = CASES[name]['accumulate'] or 1
    rows, first = [], None
    # (the float32 oracle is the NOISE yardstick: on one thread its sums have one order, so the committed table can be recomputed)
    threads = torch.get_num_threads()
    if dtype == torch.float32:
        torch.set_num_threads(1)
    try:
        for call in range(updates * k):
            o.table = table(name, call)
            l = o.batch(*inputs(name, call), train=True)
            rows.append([l[key] for key in LOSS_KEYS])
            if call == k - 1:
                first = dict(o.last)
    finally:
        torch.set_num_threads(threads)
    return dict(first=first, losses=np.array(rows), state={k_: v.clone() for k_, v in o.state().items()})


# ---------------------------------------------------------------------------------------------------------------------- distances
def l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def whole(grads, order):
    return torch.cat([torch.as_tensor(grads[k]).double().cpu().reshape(-1) for k in order])


def grad_dists(got, want):
    """{'g.<key>' | 'd.<key>': relative L2} of the closed gradients of a first update against `want`'s."""
    out = {}
    for net in ('g', 'd'):
        w = want[net + '_grads']
        assert set(got[net + '_grads']) == set(w), (sorted(got[net + '_grads']), sorted(w))
        out.update({f'{net}.{k}': l2(got[net + '_grads'][k], w[k]) for k in w})
    return out


def grad_bound(noise):
    """The standing per-parameter bound: relative L2 below 2e-2 and at most 8 x noise + 1e-3."""
    return min(2e-2, 8 * noise + 1e-3)


def largest_grad_bound(name):
    return max(8 * n + 1e-3 for n in COMBO_NOISE[name]['grad'].values())


def curve_dist(losses, state, want_losses, want_state):
    """(losses' part, state's part): the largest relative error of a loss scalar (floor 1e-6) and of a tensor (relative max-norm)."""
    losses, want_losses = np.asarray(losses, dtype=np.float64), np.asarray(want_losses, dtype=np.float64)
    e_l = float((np.abs(losses - want_losses) / np.maximum(np.abs(want_losses), 1e-6)).max())
    assert set(state) == set(want_state), (sorted(state), sorted(want_state))
    e_w = max(float((torch.as_tensor(state[k]).double().cpu() - w.double()).abs().max() / w.double().abs().max().clamp_min(1e-300))
              for k, w in want_state.items())
    return e_l, e_w


def separation(name, got_first, got_losses, got_state, other, true):
    """How far a result lies from the run `other` in units of 10 x the case's largest bound, gradients and curve: >= 1 is separated.
    -> (the larger of the two, the gradients', the curve's)."""
    worst = largest_grad_bound(name)
    far_g = max(l2(whole(got_first[n + '_grads'], true['first'][n + '_grads']), whole(other['first'][n + '_grads'], true['first'][n + '_grads']))
                for n in ('g', 'd'))
    far_c = max(curve_dist(got_losses, got_state, other['losses'], other['state']))
    rg, rc = far_g / (10 * worst), far_c / (10 * 3 * COMBO_NOISE[name]['curve'])
    return max(rg, rc), rg, rc


def hinge_sides(first):
    dr, df = first['d_real'].double(), first['d_fake'].double()
    return [float((dr < 1).double().mean()), float((dr > 1).double().mean()), float((df > -1).double().mean()), float((df < -1).double().mean())]


# ---------------------------------------------------------------------------------------------------------------------- committed tables
# The case that separates each mutation (tests/test_combo_cpu.py prints the whole table and holds these entries to >= 10 x the bound).
SEPARATES = {'fake_other_row': 'lsgan_ref', 'no_adjoint': 'hinge_shared', 'sigma_before_iteration': 'lsgan_sn', 'iterate_per_pass': 'vanilla_ce',
             'map_once_at_close': 'everything', 'clip_per_call': 'everything', 'mean_twice': 'lsgan_sn', 'weights_skip_dice': 'hinge_shared',
             'real_label_on_gen': 'lsgan_ref', 'stale_dfake': 'hinge_sn_ref',
             # (only a case whose clipped gradient keeps Adam linear has a bound these two can be seen against: see CASES)
             'decay_every_call': 'everything', 'ema_every_call': 'everything'}

# Which cases' training step takes the shared D(fake) pass (Trainer SHARE_D_FAKE: the planner's halves_ok; a discriminator with norm
# layers never does).  Recomputed from the planner by tests/test_combo_cpu.py, observed on the device by tests/test_combo_gpu.py.
SHARED = {'everything': False, 'plain': True, 'hinge_shared': True, 'hinge_sn_ref': False, 'lsgan_sn': True, 'lsgan_ce': False, 'lsgan_ref': False,
          'vanilla_sn': False, 'vanilla_ce': False, 'vanilla_accum': True}

# The float32 oracle's own distance from the float64 oracle, per case: 'curve' the one number, 'grad' per parameter of the first closed
# update.  Recomputed by tests/test_combo_cpu.py, which fails if a committed value is off by more than a factor of 2.
COMBO_NOISE = {'everything': {'curve': 2.904e-06,
                'grad': {'g.encoder.0.model.DownConv0.weight': 6.206e-06,
                         'g.encoder.1.model.DownConv1.weight': 1.364e-06,
                         'g.encoder.2.model.DownConv2.weight': 1.007e-06,
                         'g.encoder.3.model.DownConv3.weight': 9.784e-07,
                         'g.encoder.4.model.DownConv4.weight': 1.142e-06,
                         'g.encoder.5.model.DownConv5.weight': 1.322e-06,
                         'g.encoder.6.model.DownConv6.weight': 2.829e-06,
                         'g.decoder.0.model.UpConv0.weight': 1.799e-06,
                         'g.decoder.1.model.UpConv1.weight': 1.149e-06,
                         'g.decoder.2.model.UpConv2.weight': 1.097e-06,
                         'g.decoder.3.model.UpConv3.weight': 9.745e-07,
                         'g.decoder.4.model.UpConv4.weight': 1.033e-06,
                         'g.decoder.5.model.UpConv5.weight': 1.844e-06,
                         'g.decoder.6.model.UpConv6.weight': 1.315e-06,
                         'd.model.0.bias': 5.719e-06,
                         'd.model.0.weight_orig': 2.572e-06,
                         'd.model.2.weight_orig': 1.973e-06,
                         'd.model.5.weight_orig': 1.415e-06,
                         'd.model.8.weight_orig': 1.213e-06,
                         'd.model.11.weight_orig': 1.142e-06,
                         'd.model.14.weight_orig': 1.004e-06,
                         'd.model.17.bias': 4.768e-07,
                         'd.model.17.weight_orig': 8.858e-07}},
 'plain': {'curve': 0.001405,
           'grad': {'g.encoder.0.model.DownConv0.weight': 9.518e-06,
                    'g.encoder.1.model.DownConv1.weight': 1.828e-06,
                    'g.encoder.2.model.DownConv2.weight': 1.177e-06,
                    'g.encoder.3.model.DownConv3.weight': 1.102e-06,
                    'g.encoder.4.model.DownConv4.weight': 1.24e-06,
                    'g.encoder.5.model.DownConv5.weight': 1.399e-06,
                    'g.encoder.6.model.DownConv6.weight': 1.736e-06,
                    'g.decoder.0.model.UpConv0.weight': 1.095e-06,
                    'g.decoder.1.model.UpConv1.weight': 1.097e-06,
                    'g.decoder.2.model.UpConv2.weight': 9.791e-07,
                    'g.decoder.3.model.UpConv3.weight': 9.057e-07,
                    'g.decoder.4.model.UpConv4.weight': 1.108e-06,
                    'g.decoder.5.model.UpConv5.weight': 3.557e-06,
                    'g.decoder.6.model.UpConv6.weight': 2.728e-06,
                    'd.model.0.weight': 6.918e-06,
                    'd.model.0.bias': 2.609e-06,
                    'd.model.2.weight': 8.824e-06,
                    'd.model.4.weight': 3.381e-06,
                    'd.model.6.weight': 2.473e-06,
                    'd.model.8.weight': 2.452e-06,
                    'd.model.8.bias': 8.023e-05}},
 'hinge_shared': {'curve': 0.02871,
                  'grad': {'g.encoder.0.model.DownConv0.weight': 8.385e-06,
                           'g.encoder.1.model.DownConv1.weight': 1.592e-06,
                           'g.encoder.2.model.DownConv2.weight': 1.122e-06,
                           'g.encoder.3.model.DownConv3.weight': 1.071e-06,
                           'g.encoder.4.model.DownConv4.weight': 1.151e-06,
                           'g.encoder.5.model.DownConv5.weight': 1.361e-06,
                           'g.encoder.6.model.DownConv6.weight': 2.54e-06,
                           'g.decoder.0.model.UpConv0.weight': 1.668e-06,
                           'g.decoder.1.model.UpConv1.weight': 1.211e-06,
                           'g.decoder.2.model.UpConv2.weight': 1.103e-06,
                           'g.decoder.3.model.UpConv3.weight': 9.27e-07,
                           'g.decoder.4.model.UpConv4.weight': 8.289e-07,
                           'g.decoder.5.model.UpConv5.weight': 1.624e-06,
                           'g.decoder.6.model.UpConv6.weight': 2.729e-06,
                           'd.model.0.weight': 3.969e-06,
                           'd.model.0.bias': 9.451e-06,
                           'd.model.2.weight': 2.707e-06,
                           'd.model.4.weight': 2.079e-06,
                           'd.model.6.weight': 4.065e-06,
                           'd.model.8.weight': 4.824e-06,
                           'd.model.8.bias': 3.381e-05}},
 'hinge_sn_ref': {'curve': 0.0003154,
                  'grad': {'g.encoder.0.model.DownConv0.weight': 4.739e-06,
                           'g.encoder.1.model.DownConv1.weight': 1.435e-06,
                           'g.encoder.2.model.DownConv2.weight': 1.42e-06,
                           'g.encoder.3.model.DownConv3.weight': 1.486e-06,
                           'g.encoder.4.model.DownConv4.weight': 1.581e-06,
                           'g.encoder.5.model.DownConv5.weight': 1.723e-06,
                           'g.encoder.6.model.DownConv6.weight': 2.75e-06,
                           'g.decoder.0.model.UpConv0.weight': 1.585e-06,
                           'g.decoder.1.model.UpConv1.weight': 1.424e-06,
                           'g.decoder.2.model.UpConv2.weight': 1.259e-06,
                           'g.decoder.3.model.UpConv3.weight': 1.088e-06,
                           'g.decoder.4.model.UpConv4.weight': 1.006e-06,
                           'g.decoder.5.model.UpConv5.weight': 1.04e-06,
                           'g.decoder.6.model.UpConv6.weight': 1.525e-06,
                           'd.model.0.bias': 0.0005164,
                           'd.model.0.weight_orig': 0.0004043,
                           'd.model.2.weight_orig': 3.563e-06,
                           'd.model.5.weight_orig': 7.509e-07,
                           'd.model.8.weight_orig': 5.167e-07,
                           'd.model.11.bias': 3.481e-05,
                           'd.model.11.weight_orig': 5.334e-07}},
 'lsgan_sn': {'curve': 0.001629,
              'grad': {'g.encoder.0.model.DownConv0.weight': 2.796e-06,
                       'g.encoder.1.model.DownConv1.weight': 1.529e-06,
                       'g.encoder.2.model.DownConv2.weight': 1.431e-06,
                       'g.encoder.3.model.DownConv3.weight': 1.402e-06,
                       'g.encoder.4.model.DownConv4.weight': 1.479e-06,
                       'g.encoder.5.model.DownConv5.weight': 1.604e-06,
                       'g.encoder.6.model.DownConv6.weight': 2.251e-06,
                       'g.decoder.0.model.UpConv0.weight': 1.566e-06,
                       'g.decoder.1.model.UpConv1.weight': 1.443e-06,
                       'g.decoder.2.model.UpConv2.weight': 1.285e-06,
                       'g.decoder.3.model.UpConv3.weight': 1.1e-06,
                       'g.decoder.4.model.UpConv4.weight': 9.764e-07,
                       'g.decoder.5.model.UpConv5.weight': 1.051e-06,
                       'g.decoder.6.model.UpConv6.weight': 1.776e-06,
                       'd.model.0.bias': 1.053e-06,
                       'd.model.0.weight_orig': 1.818e-06,
                       'd.model.2.weight_orig': 9.459e-07,
                       'd.model.4.weight_orig': 5.392e-07,
                       'd.model.6.weight_orig': 5.613e-07,
                       'd.model.8.bias': 8.923e-07,
                       'd.model.8.weight_orig': 7.138e-07}},
 'lsgan_ce': {'curve': 0.04302,
              'grad': {'g.encoder.0.model.DownConv0.weight': 1.358e-05,
                       'g.encoder.1.model.DownConv1.weight': 1.655e-06,
                       'g.encoder.2.model.DownConv2.weight': 1.243e-06,
                       'g.encoder.3.model.DownConv3.weight': 1.358e-06,
                       'g.encoder.4.model.DownConv4.weight': 1.62e-06,
                       'g.encoder.5.model.DownConv5.weight': 1.861e-06,
                       'g.encoder.6.model.DownConv6.weight': 2.971e-06,
                       'g.decoder.0.model.UpConv0.weight': 1.353e-06,
                       'g.decoder.1.model.UpConv1.weight': 1.311e-06,
                       'g.decoder.2.model.UpConv2.weight': 1.082e-06,
                       'g.decoder.3.model.UpConv3.weight': 9.205e-07,
                       'g.decoder.4.model.UpConv4.weight': 9.902e-07,
                       'g.decoder.5.model.UpConv5.weight': 2.532e-06,
                       'g.decoder.6.model.UpConv6.weight': 1.784e-06,
                       'd.model.0.weight': 1.545e-06,
                       'd.model.0.bias': 1.134e-06,
                       'd.model.2.weight': 1.007e-06,
                       'd.model.4.weight': 5.499e-07,
                       'd.model.6.weight': 2.697e-07,
                       'd.model.8.weight': 1.929e-07,
                       'd.model.10.weight': 1.855e-07,
                       'd.model.12.weight': 1.845e-07,
                       'd.model.12.bias': 5.687e-08}},
 'lsgan_ref': {'curve': 0.000573,
               'grad': {'g.encoder.0.model.DownConv0.weight': 1.754e-05,
                        'g.encoder.1.model.DownConv1.weight': 2.039e-06,
                        'g.encoder.2.model.DownConv2.weight': 1.475e-06,
                        'g.encoder.3.model.DownConv3.weight': 1.592e-06,
                        'g.encoder.4.model.DownConv4.weight': 1.97e-06,
                        'g.encoder.5.model.DownConv5.weight': 2.195e-06,
                        'g.encoder.6.model.DownConv6.weight': 8.01e-06,
                        'g.decoder.0.model.UpConv0.weight': 2.303e-06,
                        'g.decoder.1.model.UpConv1.weight': 1.046e-06,
                        'g.decoder.2.model.UpConv2.weight': 9.453e-07,
                        'g.decoder.3.model.UpConv3.weight': 8.814e-07,
                        'g.decoder.4.model.UpConv4.weight': 1.085e-06,
                        'g.decoder.5.model.UpConv5.weight': 2.159e-06,
                        'g.decoder.6.model.UpConv6.weight': 2.76e-06,
                        'd.model.0.weight': 1.921e-06,
                        'd.model.0.bias': 1.293e-06,
                        'd.model.2.weight': 1.185e-06,
                        'd.model.5.weight': 6.435e-07,
                        'd.model.8.weight': 6.291e-07,
                        'd.model.11.weight': 1.023e-06,
                        'd.model.11.bias': 1.462e-06}},
 'vanilla_sn': {'curve': 0.002981,
                'grad': {'g.encoder.0.model.DownConv0.weight': 4.646e-06,
                         'g.encoder.1.model.DownConv1.weight': 2.061e-06,
                         'g.encoder.2.model.DownConv2.weight': 2.179e-06,
                         'g.encoder.3.model.DownConv3.weight': 2.52e-06,
                         'g.encoder.4.model.DownConv4.weight': 2.835e-06,
                         'g.encoder.5.model.DownConv5.weight': 3.323e-06,
                         'g.encoder.6.model.DownConv6.weight': 7.857e-06,
                         'g.decoder.0.model.UpConv0.weight': 2.198e-06,
                         'g.decoder.1.model.UpConv1.weight': 1.814e-06,
                         'g.decoder.2.model.UpConv2.weight': 1.576e-06,
                         'g.decoder.3.model.UpConv3.weight': 1.353e-06,
                         'g.decoder.4.model.UpConv4.weight': 1.261e-06,
                         'g.decoder.5.model.UpConv5.weight': 1.36e-06,
                         'g.decoder.6.model.UpConv6.weight': 2.229e-06,
                         'd.model.0.bias': 5.524e-06,
                         'd.model.0.weight_orig': 4.096e-06,
                         'd.model.2.weight_orig': 2.852e-06,
                         'd.model.5.weight_orig': 8.908e-07,
                         'd.model.8.weight_orig': 6.453e-07,
                         'd.model.11.bias': 5.67e-05,
                         'd.model.11.weight_orig': 7.817e-07}},
 'vanilla_ce': {'curve': 0.04426,
                'grad': {'g.encoder.0.model.DownConv0.weight': 4.997e-06,
                         'g.encoder.1.model.DownConv1.weight': 1.345e-06,
                         'g.encoder.2.model.DownConv2.weight': 1.04e-06,
                         'g.encoder.3.model.DownConv3.weight': 1.012e-06,
                         'g.encoder.4.model.DownConv4.weight': 1.169e-06,
                         'g.encoder.5.model.DownConv5.weight': 1.348e-06,
                         'g.encoder.6.model.DownConv6.weight': 2.728e-06,
                         'g.decoder.0.model.UpConv0.weight': 1.512e-06,
                         'g.decoder.1.model.UpConv1.weight': 1.152e-06,
                         'g.decoder.2.model.UpConv2.weight': 1.066e-06,
                         'g.decoder.3.model.UpConv3.weight': 1.013e-06,
                         'g.decoder.4.model.UpConv4.weight': 9.692e-07,
                         'g.decoder.5.model.UpConv5.weight': 2.102e-06,
                         'g.decoder.6.model.UpConv6.weight': 1.399e-06,
                         'd.model.0.bias': 1.432e-05,
                         'd.model.0.weight_orig': 6.522e-06,
                         'd.model.2.weight_orig': 4.538e-06,
                         'd.model.4.weight_orig': 2.654e-06,
                         'd.model.6.weight_orig': 1.718e-06,
                         'd.model.8.weight_orig': 1.155e-06,
                         'd.model.10.weight_orig': 1.236e-06,
                         'd.model.12.bias': 7.996e-06,
                         'd.model.12.weight_orig': 1.187e-06}},
 'vanilla_accum': {'curve': 0.0006072,
                   'grad': {'g.encoder.0.model.DownConv0.weight': 1.985e-05,
                            'g.encoder.1.model.DownConv1.weight': 1.809e-06,
                            'g.encoder.2.model.DownConv2.weight': 1.303e-06,
                            'g.encoder.3.model.DownConv3.weight': 1.272e-06,
                            'g.encoder.4.model.DownConv4.weight': 1.479e-06,
                            'g.encoder.5.model.DownConv5.weight': 1.774e-06,
                            'g.encoder.6.model.DownConv6.weight': 3.659e-06,
                            'g.decoder.0.model.UpConv0.weight': 1.503e-06,
                            'g.decoder.1.model.UpConv1.weight': 1.332e-06,
                            'g.decoder.2.model.UpConv2.weight': 1.195e-06,
                            'g.decoder.3.model.UpConv3.weight': 1.115e-06,
                            'g.decoder.4.model.UpConv4.weight': 1.189e-06,
                            'g.decoder.5.model.UpConv5.weight': 2.215e-06,
                            'g.decoder.6.model.UpConv6.weight': 1.852e-06,
                            'd.model.0.weight': 7.934e-06,
                            'd.model.0.bias': 0.0001661,
                            'd.model.2.weight': 5.45e-06,
                            'd.model.4.weight': 2.787e-06,
                            'd.model.6.weight': 2.548e-06,
                            'd.model.8.weight': 3.439e-06,
                            'd.model.8.bias': 2.658e-05}}}
