"""References, tolerances and the oracle trainer for the GAN objectives (Trainer.gan_mode; pg_gan_loss of ganloss.hip).  Pure CPU: torch
+ numpy, nothing here calls the library.

A term is a mean over the n = N * HW values d of a one-channel patch map, e(d) by kind (include/patchgan_hip.h):
  lsgan        e = (d - t)^2                          de/dd = 2 (d - t)
  hinge_d      t = 1: e = max(0, 1 - d)               de/dd = -1 where 1 - d > 0 else 0
               t = 0: e = max(0, 1 + d)               de/dd = +1 where 1 + d > 0 else 0
  hinge_g      e = -d                                 de/dd = -1
  bce_logits   e = max(d, 0) - d t + log1p(exp(-|d|))   de/dd = sigmoid(d) - t
value = scale * sum e, g = scale * de/dd, scale = alpha / (Bglobal * HW).  The float64 references evaluate these expressions on the stored
fp32 values (d and t are values representable in fp32); tests/test_ganloss_cpu.py holds them to torch's F.mse_loss, F.relu and
F.binary_cross_entropy_with_logits and their autograd.  The "plain fp32" evaluation does every element operation in fp32 NumPy and
the sum in fp64 (an emulation of no particular kernel); it decides whether a bound is sound and carries the mutations the comparator
must reject.

Tolerances (the convention of tests/lossopt_util.py: eps32 = 2^-23 per rounding, although one costs at most half of it; TINY = 2^-126;
n 2^-52 for the fp64 accumulation; expf and log1pf documented at 1 ulp = one rounding each):
  element e    lsgan       3 eps32 e                    d - t (entering the square twice), the product
               hinge_d     eps32 |1 -+ d| where active  the one difference; the SIGN of an fp32 difference is exact, so the active set is
               hinge_g     0                            a negation is exact
               bce_logits  eps32 (|d t| + |max(d, 0) - d t| + 2 l + |e|),  l = log1p(exp(-|d|)):  the product, the difference, expf
                           (|d log1p(x)| <= x / (1 + x) |dx / x| <= l |dx / x|) and log1pf, the last sum
               each + TINY (exp(-|d|) is subnormal beyond |d| = 87.3: kept or flushed)
  value        scale (sum tol_e + n 2^-52 sum |e|) + eps32 |value| + TINY      (the one rounding to float of the fp64 product)
  gradient     lsgan       3 eps32 |g| + TINY           d - t, fl32(scale), the product (2 a is exact)
               hinge_d, hinge_g   bit equality with +-fl32(scale) or 0
               bce_logits  |sf| (4 eps32 s + eps32 |s - t|) + 2 eps32 |g| + TINY,  s = sigmoid(d):  expf, 1 + x, the division (and
                           the numerator x on the negative side): four on s; s - t; fl32(scale) and the product
A NaN in d is checked apart (value and that element's gradient are NaN in every kind); the inputs here are finite."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.patchgan_oracle import OracleTrainer, adam_update, apply_act, bce, disc_plan, instance_norm, seg_loss
from tests.diffaug_util import AugOracleTrainer, apply_torch

EPS32 = 2.0 ** -23
TINY = 2.0 ** -126
ACC = 2.0 ** -52
LSGAN, HINGE_D, HINGE_G, BCE_LOGITS = 0, 1, 2, 3          # PG_GAN_*
KINDS = {'lsgan': LSGAN, 'hinge_d': HINGE_D, 'hinge_g': HINGE_G, 'bce_logits': BCE_LOGITS}
GAN_MODES = ('vanilla', 'lsgan', 'hinge')
# planted among random values in +-4: both zeros, the margins and their fp32 neighbours, the smallest subnormal, large values of both signs
PLANTED = (0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, -(1.0 + 2.0 ** -23), -(1.0 - 2.0 ** -23), 2.0 ** -149,
           1e4, -1e4, 90.0, -90.0)


def f32(x):
    """The float64 value of x rounded to fp32."""
    return float(np.float32(x))


def patch_values(n, seed):
    """n fp32 values: uniform in +-4 with PLANTED written over the first places (as many as fit), as a float32 array."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    k = min(n, len(PLANTED))
    d[:k] = np.array(PLANTED, dtype=np.float32)[:k]
    return d


def scale_of(alpha, bglobal, hw):
    return float(alpha) / (float(bglobal) * float(hw))


# ---- float64 references ------------------------------------------------------------------------------------------------------------------

def elem_ref(kind, d, t):
    """(e, de/dd) in float64 from an array of fp32-representable values."""
    d = np.asarray(d, dtype=np.float64)
    t = f32(t)
    if kind == LSGAN:
        a = d - t
        return a * a, 2.0 * a
    if kind == HINGE_D:
        assert t in (0.0, 1.0)
        a = 1.0 - d if t == 1.0 else 1.0 + d
        return np.where(a > 0, a, 0.0), np.where(a > 0, -1.0 if t == 1.0 else 1.0, 0.0)
    if kind == HINGE_G:
        return -d, np.full_like(d, -1.0)
    assert kind == BCE_LOGITS
    ex = np.exp(-np.abs(d))
    s = np.where(d >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))
    return np.maximum(d, 0.0) - d * t + np.log1p(ex), s - t


def term_ref(kind, d, t, scale):
    """(value, gradient) of one term in float64: scale * sum e, scale * de/dd."""
    e, de = elem_ref(kind, d, t)
    return float(scale * e.sum()), scale * de


def term_torch(kind, d, t, scale):
    """The same through the functions the issue names and their autograd: float64 torch."""
    x = torch.tensor(np.asarray(d, dtype=np.float64), requires_grad=True)
    tt = torch.full_like(x, f32(t))
    if kind == LSGAN:
        s = F.mse_loss(x, tt, reduction='sum')
    elif kind == HINGE_D:
        s = F.relu(1.0 - x).sum() if f32(t) == 1.0 else F.relu(1.0 + x).sum()
    elif kind == HINGE_G:
        s = -x.sum()
    else:
        s = F.binary_cross_entropy_with_logits(x, tt, reduction='sum')
    v = scale * s
    g, = torch.autograd.grad(v, x)
    return float(v.detach()), g.numpy()


# ---- tolerances --------------------------------------------------------------------------------------------------------------------------

def tolerances(kind, d, t, scale):
    """(tol_value, tol_grad per element or None where the gradient is held to bit equality)."""
    d = np.asarray(d, dtype=np.float64)
    t = f32(t)
    e, de = elem_ref(kind, d, t)
    n, sf = d.size, abs(f32(scale))
    if kind == LSGAN:
        tol_e = 3 * EPS32 * e + TINY
        tol_g = 3 * EPS32 * np.abs(scale * de) + TINY
    elif kind == HINGE_D:
        tol_e = EPS32 * e + TINY
        tol_g = None
    elif kind == HINGE_G:
        tol_e = np.zeros_like(e)
        tol_g = None
    else:
        ex = np.exp(-np.abs(d))
        l, pos = np.log1p(ex), np.maximum(d, 0.0)
        tol_e = EPS32 * (np.abs(d * t) + np.abs(pos - d * t) + 2 * l + np.abs(e)) + TINY
        s = de + t
        tol_g = sf * (4 * EPS32 * s + EPS32 * np.abs(de)) + 2 * EPS32 * np.abs(scale * de) + TINY
    value = scale * e.sum()
    tol_v = abs(scale) * (tol_e.sum() + n * ACC * np.abs(e).sum()) + EPS32 * abs(value) + TINY
    return float(tol_v), tol_g


def ratios(kind, d, t, scale, value, grad):
    """How far (value, grad) -- a float and an fp32 array or None -- lie from the float64 reference, in units of the bound: (value ratio,
    gradient ratio).  A gradient held to bit equality gives 0.0 or inf.  <= 1.0 passes."""
    want_v, want_g = term_ref(kind, d, t, scale)
    tol_v, tol_g = tolerances(kind, d, t, scale)
    rv = abs(float(value) - want_v) / tol_v
    if grad is None:
        return rv, 0.0
    grad = np.asarray(grad)
    if tol_g is None:
        de = elem_ref(kind, d, t)[1]
        want = np.float32(scale) * de.astype(np.float32)          # (+-1 or 0 times fl32(scale): exact)
        same = np.array_equal(grad.astype(np.float32), want)     # (values equal; the sign of a zero is not held)
        return rv, 0.0 if same else float('inf')
    return rv, float((np.abs(grad.astype(np.float64) - want_g) / tol_g).max())


# ---- the plain fp32 evaluation, with the mutations the comparator must reject ----------------------------------------------------------

MUTATIONS = ('hinge_sign', 'hinge_ge', 'lsgan_no2', 'naive_softplus')


def term_fp32(kind, d, t, scale, mutate=None):
    """(value as np.float32, gradient as a float32 array): element arithmetic in fp32, the sum in fp64, one rounding of the value."""
    d = np.asarray(d, dtype=np.float32)
    t, sf, one = np.float32(t), np.float32(scale), np.float32(1.0)
    with np.errstate(over='ignore', invalid='ignore'):
        if kind == LSGAN:
            a = d - t
            e, de = a * a, (one if mutate == 'lsgan_no2' else np.float32(2.0)) * a
        elif kind == HINGE_D:
            real = t != 0
            a = one - d if real else one + d
            act = (a >= 0) if mutate == 'hinge_ge' else (a > 0)
            sign = np.float32(-1.0 if real else 1.0) * (np.float32(-1.0) if mutate == 'hinge_sign' else one)
            e, de = np.where(act, a, np.float32(0.0)), np.where(act, sign, np.float32(0.0))
        elif kind == HINGE_G:
            e, de = -d, np.full_like(d, -1.0 if mutate != 'hinge_sign' else 1.0)
        else:
            ex = np.exp(-np.abs(d)).astype(np.float32)
            pos = np.maximum(d, np.float32(0.0))
            if mutate == 'naive_softplus':          # log(1 + exp(d)) - d t: overflows beyond d = 88.7
                e = np.log(one + np.exp(d).astype(np.float32)).astype(np.float32) - d * t
            else:
                e = (pos - d * t) + np.log1p(ex).astype(np.float32)
            s = np.where(d >= 0, one / (one + ex), ex / (one + ex)).astype(np.float32)
            de = s - t
    value = np.float32(float(scale) * float(e.astype(np.float64).sum()))
    return value, (sf * de.astype(np.float32)).astype(np.float32)


# ---- what a step asks of the kernel --------------------------------------------------------------------------------------------------------

def step_terms(gan_mode, final_act, real_label=1.0):
    """{'gen' | 'real' | 'fake': (kind name, target, alpha)} of one step; None for vanilla on a sigmoid head (the BCE kernels)."""
    if gan_mode == 'hinge':
        return dict(gen=('hinge_g', 1.0, 1.0), real=('hinge_d', 1.0, 0.5), fake=('hinge_d', 0.0, 0.5))
    if gan_mode == 'vanilla' and final_act == 'sigmoid':
        return None
    k = 'lsgan' if gan_mode == 'lsgan' else 'bce_logits'
    return dict(gen=(k, 1.0, 1.0), real=(k, real_label, 0.5), fake=(k, 0.0, 0.5))


# ---- the oracle trainer ------------------------------------------------------------------------------------------------------------------

class GanOracleTrainer(OracleTrainer):
    """OracleTrainer with the objective of Trainer.gan_mode / real_label and, with d_final_act = 'none', a discriminator without its
    last activation.  The defaults are OracleTrainer, operation for operation."""

    gan_mode = 'vanilla'
    real_label = 1.0
    d_final_act = 'sigmoid'

    def pre_D(self, x):
        return x

    def D(self, x, probes=None):
        if self.d_final_act == 'sigmoid':
            return super().D(x, probes)
        x = self.pre_D(x)
        h = x
        plan = disc_plan(x.shape[1], self.dw['model.0.weight'].shape[0], self.n_layers, self.norm)
        for li, (idx, _cin, _cout, stride, bias, act, has_norm) in enumerate(plan):
            h = F.conv2d(h, self.dw[f'model.{idx}.weight'], self.dw[f'model.{idx}.bias'] if bias else None, stride=stride, padding=1)
            h = apply_act(h, act if li < len(plan) - 1 else 'none')
            if has_norm:
                h = instance_norm(h)
        return h

    def _gdisc(self, d_fake):
        if self.gan_mode == 'hinge':
            return -torch.mean(d_fake)
        if self.gan_mode == 'lsgan':
            return F.mse_loss(d_fake, torch.ones_like(d_fake))
        if self.d_final_act == 'none':
            return F.binary_cross_entropy_with_logits(d_fake, torch.ones_like(d_fake))
        return bce(d_fake, torch.ones_like(d_fake))

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

    def batch(self, x, y, train=False, dropout_masks=None):
        assert self.gan_mode in GAN_MODES and self.d_final_act in ('sigmoid', 'none')
        x = x.to(self.dtype)
        y = y.to(self.dtype)
        gen_img = self.G(x, dropout_masks)
        disc_fake = self.D(torch.cat((x, gen_img), 1))
        gen_loss_seg = seg_loss(self.loss_type, gen_img, y, self.seg_alpha, self.beta, self.gamma)
        gen_loss_disc = self._gdisc(disc_fake)
        gen_loss = gen_loss_seg + gen_loss_disc
        if train:
            names = list(self.gw)
            grads = torch.autograd.grad(gen_loss, [self.gw[k] for k in names])
            self.last['g_grads'] = dict(zip(names, grads))
            self.t_g += 1
            with torch.no_grad():
                for k, g in zip(names, grads):
                    adam_update(self.gw[k], g, self.gm[k], self.gv[k], self.t_g, self.gen_lr)
        disc_real = self.D(torch.cat((x, y), 1))
        disc_fake2 = self.D(torch.cat((x, gen_img.detach()), 1))
        self.last['d_real'], self.last['d_fake'] = disc_real.detach(), disc_fake2.detach()
        loss_real, loss_fake = self._real_fake(disc_real, disc_fake2)
        disc_loss = (loss_fake + loss_real) / 2.
        if train:
            names = list(self.dw)
            grads = torch.autograd.grad(disc_loss, [self.dw[k] for k in names])
            self.last['d_grads'] = dict(zip(names, grads))
            self.t_d += 1
            with torch.no_grad():
                for k, g in zip(names, grads):
                    adam_update(self.dw[k], g, self.dm[k], self.dv[k], self.t_d, self.dsc_lr)
        self.last['gen_img'] = gen_img.detach()
        vals = [gen_loss.item(), gen_loss.item(), gen_loss_disc.item(), loss_real.item(), loss_fake.item(), disc_loss.item()]
        return dict(zip(self.keys, vals))


class GanAugOracleTrainer(GanOracleTrainer, AugOracleTrainer):
    """... whose discriminator reads T(x | y) and T(x | G(x)) (AugOracleTrainer.table) under either head."""

    def pre_D(self, x):
        return apply_torch(x, self.table) if self.table is not None else x


def gan_oracle(gold, dtype, gan_mode='vanilla', real_label=1.0, d_final_act='sigmoid', head_gain=1.0, **kw):
    """GanOracleTrainer on a golden fixture's networks; head_gain multiplies the head conv's weight (model.8.weight of the three-layer
    fixtures: spreads the logits over the hinge margins)."""
    c = gold.cfg
    args = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=c['loss_type'],
                dtype=dtype)
    args.update(kw)
    dw = gold.weights('d0')
    if head_gain != 1.0:
        dw[head_key(dw)] = dw[head_key(dw)] * head_gain
    o = GanOracleTrainer(gold.weights('g0'), dw, **args)
    o.gan_mode, o.real_label, o.d_final_act = gan_mode, real_label, d_final_act
    return o


def head_key(dw):
    """The head conv's weight key: the highest model.{i}.weight."""
    return max((k for k in dw if k.endswith('.weight')), key=lambda k: int(k.split('.')[1]))
