"""References, tolerances, inputs and the oracle trainer for the segmentation objectives beyond the reference's three
(Trainer.loss_type = 'ce' | 'focal' | 'dice' and their '+'-joined sums; pg_seg_loss_reduce / pg_seg_loss_value_grad of segloss.hip).
Pure CPU: torch + numpy, nothing here calls the library.

Tensors are float64 torch tensors of shape (N, HW, C) holding values representable in fp32.  With p the prediction, y the target,
  lp = max(log p, -100), lq = max(log1p(-p), -100), q = 1 - p, x^k = x^(k-1) x from x^0 = 1, g = focal_gamma (an integer in 0..8),
  a1 = fl32(focal_alpha), a0 = fl32(1 - a1) (both 1 for focal_alpha None), CLAMP = fl32(1e-12), s = fl32(dice_smooth), B = Bglobal:
  ce     e = -y lp                                       de/dp = -y / max(p, CLAMP)          value alpha / (B HW) sum e
  focal  e = -(a1 y q^g lp + a0 (1 - y) p^g lq)          de/dp = -a1 y (q^g / max(p, CLAMP) - g q^(g-1) lp)
                                                                 - a0 (1 - y) (g p^(g-1) lq - p^g / max(q, CLAMP))
                                                         (g = 0: the g ... terms are absent)  value alpha / (B C HW) sum e
  dice   I = sum p y, P = sum p, Y = sum y over HW, D = (2 I + s) / (P + Y + s)                value alpha / (B C) sum_{n,c} (1 - D)
         gradient k0 y + k1 with (k0, k1) = d value / d (I, P): float64 autograd of the value as a function of the three sums
A sum's value and gradient are the sums of its members'.  The float64 references evaluate these definitions on the stored values; the
gradients of ce and focal ARE the definitions (they carry the CLAMP, which the derivative of the clamped value does not), and
tests/test_segloss_cpu.py holds them to float64 autograd away from the clamps.  The "plain fp32" evaluation does every element operation
in fp32 NumPy in the order the header writes it and the sums in fp64 (an emulation of no particular kernel); it decides whether a bound
is sound and carries the mutations the comparator must reject.

Tolerances (the convention of tests/lossopt_util.py: eps32 = 2^-23 per rounding counted, although one costs at most half of it;
TINY = 2^-126; n 2^-52 for an fp64 accumulation of n terms; 2^-40 relative for a handful of fp64 operations; logf and log1pf at their
documented 1 ulp = one rounding each).  Roundings per expression, with t1 = a1 y q^g lp, t0 = a0 (1 - y) p^g lq:
  lp, lq        1 each (the clamp is exact)
  x^k           p is stored: k - 1 products.  q = fl(1 - p) carries one rounding into each of the k factors: 2k - 1 (0 for k = 0).
  ce e          2: lp, the product                                             tol 2 eps32 |e| + TINY
  ce g          3: the division, fl32(scale), the product                      tol 3 eps32 |g| + TINY
  focal e       t1: a1 y, q^g (2g - 1), the product, lp, the product: <= 4 + 2g;  t0: 1 - y, a0 (1 - y), p^g (g - 1), the product,
                lq, the product: <= 5 + g;  the sum of the two: 1 on each       tol eps32 ((5 + 2g) |t1| + (6 + g) |t0|) + 2^8 TINY
                (a product that leaves the normal range is off by at most TINY, and at most |log| <= 100 multiplies it afterwards)
  focal g       A = q^g / max(p, CLAMP) - (g q^(g-1)) lp: either term <= 2g roundings, the difference 1: (2g + 1) eps32 (|A1| + |A2|);
                B = (g p^(g-1)) lq - p^g / max(q, CLAMP): either term <= g + 1 (q's rounding enters the divisor), the difference 1:
                (g + 2) eps32 (|B1| + |B2|);  u1 = (a1 y) A: 2 more;  u0 = (a0 (1 - y)) B: 3 more;  u1 + u0: 1 on each;  fl32(scale)
                and the product: 2.   tol |sf| (|a1 y| tol_A + |a0 (1 - y)| tol_B + 5 eps32 |u1| + 6 eps32 |u0|) + 2^10 TINY max(1, |sf|)
                (g <= 8 and |log| <= 100 multiply a flushed intermediate by at most 800)
  dice sums     I: 1 (the product) -> eps32 sum |p y| + HW 2^-52 sum |p y| + HW TINY;  P, Y: stored values, HW 2^-52 of the sum
  dice value    sum |d value / d S| tol_S (autograd) + 2^-40 |value|
  dice k0, k1   eps32 |k| (the one rounding) + 2^-40 |k| + sum |d k / d S| tol_S (the autograd Jacobian of (k0, k1) in the sums)
  dice g        k0 y + k1: 2 (product, sum)                                    tol 2 eps32 (|k0 y| + |k1|) + |y| tol_k0 + tol_k1 + TINY
  value         sum over members of scale (sum tol_e + n 2^-52 sum |e|) (dice: its own tolerance) + (eps32 + 2^-40) sum |member value|
                + TINY: the fp64 products and sums and the one rounding to float
  gradient      the members' tolerances + eps32 sum |member gradient| for each of the (members - 1) fp32 additions + TINY
A NaN in p is checked apart; the inputs here keep every reference value finite, which the references assert."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.patchgan_oracle import OracleTrainer, adam_update, bce
from tests.normact_util import EPS32

F64 = torch.float64
TINY = 2.0 ** -126
ACC = 2.0 ** -52
REL64 = 2.0 ** -40
CE, FOCAL, DICE = 1, 2, 4          # PG_SEG_*
BITS = {'ce': CE, 'focal': FOCAL, 'dice': DICE}
ALPHA_NONE = -1.0                  # PG_SEG_FOCAL_ALPHA_NONE
CLAMP = float(np.float32(1e-12))
PLANTED_P = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 2.0 ** -149)


def f32(x):
    return float(np.float32(x))


class Settings:
    """One evaluation's settings as the entry points take them: the term mask, focal_gamma, focal_alpha (None = none), dice_smooth,
    seg_alpha and the global batch."""

    def __init__(self, terms, gamma=2, focal_alpha=None, smooth=1.0, alpha=200.0, bglobal=None):
        self.terms = sum(BITS[m] for m in terms.split('+')) if isinstance(terms, str) else int(terms)
        self.gamma, self.focal_alpha, self.smooth, self.alpha, self.bglobal = int(gamma), focal_alpha, f32(smooth), float(alpha), bglobal
        self.a1 = 1.0 if focal_alpha is None else f32(focal_alpha)
        self.a0 = 1.0 if focal_alpha is None else f32(np.float32(1.0) - np.float32(focal_alpha))

    def members(self):
        return [m for m in ('ce', 'focal', 'dice') if self.terms & BITS[m]]

    def scales(self, N, HW, C):
        """(scale_ce, scale_focal, scale_dice) as the caller forms them in double."""
        b = float(self.bglobal if self.bglobal is not None else N)
        return self.alpha / (b * HW), self.alpha / (b * C * HW), self.alpha / (b * C)

    def alpha_arg(self):
        return ALPHA_NONE if self.focal_alpha is None else float(self.focal_alpha)


def ipow(x, k):
    out = torch.ones_like(x)
    for _ in range(k):
        out = out * x
    return out


# ---- float64 references ------------------------------------------------------------------------------------------------------------------

def logs(p):
    return torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)


def ce_elem(p, y):
    lp, _ = logs(p)
    return -(y * lp)


def ce_dedp(p, y):
    return -y / p.clamp_min(CLAMP)


def focal_parts(p, y, st):
    """(t1, t0) with e = -(t1 + t0)."""
    lp, lq = logs(p)
    q = 1.0 - p
    return st.a1 * y * ipow(q, st.gamma) * lp, st.a0 * (1.0 - y) * ipow(p, st.gamma) * lq


def focal_elem(p, y, st):
    t1, t0 = focal_parts(p, y, st)
    return -(t1 + t0)


def focal_grad_parts(p, y, st):
    """(A1, A2, B1, B2) with A = A1 - A2, B = B2 - B1 and de/dp = -(a1 y A + a0 (1 - y) B)."""
    lp, lq = logs(p)
    q, g = 1.0 - p, st.gamma
    A1, B1 = ipow(q, g) / p.clamp_min(CLAMP), ipow(p, g) / q.clamp_min(CLAMP)
    if g > 0:
        A2, B2 = g * ipow(q, g - 1) * lp, g * ipow(p, g - 1) * lq
    else:
        A2, B2 = torch.zeros_like(p), torch.zeros_like(p)
    return A1, A2, B1, B2


def focal_dedp(p, y, st):
    A1, A2, B1, B2 = focal_grad_parts(p, y, st)
    return -(st.a1 * y * (A1 - A2) + st.a0 * (1.0 - y) * (B2 - B1))


def dice_sums(p, y):
    """(N, C, 3): I, P, Y over HW."""
    return torch.stack([(p * y).sum(1), p.sum(1), y.sum(1)], -1)


def dice_of_sums(S, smooth):
    """sum_{n,c} (1 - D) as a function of the sums (N, C, 3)."""
    return (1.0 - (2.0 * S[..., 0] + smooth) / (S[..., 1] + S[..., 2] + smooth)).sum()


def dice_coef(S, scale, smooth, create_graph=False):
    """(k0, k1) (N, C, 2) = d (scale sum (1 - D)) / d (I, P): autograd in the sums."""
    dS, = torch.autograd.grad(scale * dice_of_sums(S, smooth), S, create_graph=create_graph)
    return dS[..., :2]


def reference(p, y, st):
    """{'value': float, 'grad': (N, HW, C), 'members': {name: (value, grad)}} in float64."""
    N, HW, C = p.shape
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    out = {}
    if st.terms & CE:
        out['ce'] = (sc_ce * ce_elem(p, y).sum(), sc_ce * ce_dedp(p, y))
    if st.terms & FOCAL:
        out['focal'] = (sc_focal * focal_elem(p, y, st).sum(), sc_focal * focal_dedp(p, y, st))
    if st.terms & DICE:
        S = dice_sums(p, y).requires_grad_(True)
        k = dice_coef(S, sc_dice, st.smooth).detach()
        out['dice'] = (sc_dice * dice_of_sums(S.detach(), st.smooth), k[..., 0].unsqueeze(1) * y + k[..., 1].unsqueeze(1))
    value, grad = sum(v for v, _ in out.values()), sum(g for _, g in out.values())
    assert bool(torch.isfinite(value)) and bool(torch.isfinite(grad).all()), 'the inputs must keep the references finite'
    return {'value': float(value), 'grad': grad, 'members': out}


def loss_of_p(p, y, st):
    """The value as a differentiable float64 expression of p (for autograd checks away from the clamps)."""
    N, HW, C = p.shape
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    v = 0.0
    if st.terms & CE:
        v = v + sc_ce * ce_elem(p, y).sum()
    if st.terms & FOCAL:
        v = v + sc_focal * focal_elem(p, y, st).sum()
    if st.terms & DICE:
        v = v + sc_dice * dice_of_sums(dice_sums(p, y), st.smooth)
    return v


# ---- tolerances --------------------------------------------------------------------------------------------------------------------------

def tolerances(p, y, st):
    """(tol_value, tol_grad (N, HW, C)) of the evaluation."""
    N, HW, C = p.shape
    n = N * HW * C
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    g = st.gamma
    tol_v, mag_v = 0.0, 0.0
    tol_g, mag_g, members = torch.zeros_like(p), torch.zeros_like(p), 0
    if st.terms & CE:
        e, gr = ce_elem(p, y), sc_ce * ce_dedp(p, y)
        tol_v += sc_ce * float((2 * EPS32 * e.abs() + TINY).sum() + n * ACC * e.abs().sum())
        mag_v += sc_ce * float(e.abs().sum())
        tol_g, mag_g, members = tol_g + 3 * EPS32 * gr.abs() + TINY, mag_g + gr.abs(), members + 1
    if st.terms & FOCAL:
        t1, t0 = focal_parts(p, y, st)
        tol_e = EPS32 * ((5 + 2 * g) * t1.abs() + (6 + g) * t0.abs()) + 2 ** 8 * TINY
        mag = (t1.abs() + t0.abs()).sum()
        tol_v += sc_focal * float(tol_e.sum() + n * ACC * mag)
        mag_v += sc_focal * float(mag)
        A1, A2, B1, B2 = focal_grad_parts(p, y, st)
        w1, w0 = (st.a1 * y).abs(), (st.a0 * (1.0 - y)).abs()
        tol_A, tol_B = (2 * g + 1) * EPS32 * (A1.abs() + A2.abs()), (g + 2) * EPS32 * (B1.abs() + B2.abs())
        u1, u0 = w1 * (A1 - A2).abs(), w0 * (B2 - B1).abs()
        sf = abs(sc_focal)
        tol_g = tol_g + sf * (w1 * tol_A + w0 * tol_B + 5 * EPS32 * u1 + 6 * EPS32 * u0) + 2 ** 10 * TINY * max(1.0, sf)
        mag_g, members = mag_g + sf * (u1 + u0), members + 1
    if st.terms & DICE:
        S = dice_sums(p, y).requires_grad_(True)
        py = (p * y).abs().sum(1)
        tol_S = torch.stack([EPS32 * py + HW * ACC * py + HW * TINY, HW * ACC * S[..., 1].detach().abs(), HW * ACC * S[..., 2].detach().abs()], -1)
        val = sc_dice * dice_of_sums(S, st.smooth)
        dS, = torch.autograd.grad(val, S)
        tol_v += float((dS.abs() * tol_S).sum()) + REL64 * abs(float(val.detach()))
        mag_v += abs(float(val.detach()))
        k = dice_coef(S, sc_dice, st.smooth).detach()
        J = torch.autograd.functional.jacobian(lambda s: dice_coef(s, sc_dice, st.smooth, True), S.detach().clone().requires_grad_(True))
        tol_k = (EPS32 + REL64) * k.abs() + (J.abs() * tol_S).sum((-1, -2, -3))
        k0y, k1 = (k[..., 0].unsqueeze(1) * y).abs(), k[..., 1].unsqueeze(1).abs().expand_as(p)
        tol_g = tol_g + 2 * EPS32 * (k0y + k1) + y.abs() * tol_k[..., 0].unsqueeze(1) + tol_k[..., 1].unsqueeze(1) + TINY
        mag_g, members = mag_g + k0y + k1, members + 1
    tol_v += (EPS32 + REL64) * mag_v + TINY
    tol_g = tol_g + (members - 1) * EPS32 * mag_g + TINY
    return float(tol_v), tol_g


class Expect:
    """The float64 reference and the tolerances of one evaluation, computed once and shared by every call held to them."""

    def __init__(self, p, y, st):
        self.shape, self.ref = tuple(p.shape), reference(p, y, st)
        self.tol_v, self.tol_g = tolerances(p, y, st)

    def ratios(self, value, grad):
        """How far (value, grad) -- a float and an (N, HW, C) array or None -- lie from the reference in units of the bound: (value
        ratio, worst gradient ratio).  <= 1.0 passes; a NaN counts as inf."""
        rv = abs(float(value) - self.ref['value']) / self.tol_v
        rv = float('inf') if rv != rv else rv
        if grad is None:
            return rv, 0.0
        got = torch.as_tensor(np.asarray(grad), dtype=F64).reshape(self.shape)
        r = (got - self.ref['grad']).abs() / self.tol_g
        r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
        return rv, float(r.max())


def ratios(p, y, st, value, grad):
    return Expect(p, y, st).ratios(value, grad)


# ---- the plain fp32 evaluation, with the mutations the comparator must reject -----------------------------------------------------------

MUTATIONS = ('dice_no_smooth_num', 'dice_k1_sign', 'focal_no_g_term', 'focal_swap_alpha', 'ce_norm_chw', 'ce_no_clamp')


def _ipow32(x, k):
    lo = np.ones_like(x)
    for _ in range(1, k):
        lo = lo * x
    return lo, (lo * x if k > 0 else np.ones_like(x))


def plain_fp32(p, y, st, mutate=None):
    """(value as np.float32, gradient as a float32 array (N, HW, C)): element arithmetic in fp32 in the header's order, sums and Dice
    coefficients in fp64, the members' gradients rounded to fp32 and added in fp32."""
    N, HW, C = p.shape
    p32, y32 = p.numpy().astype(np.float32), y.numpy().astype(np.float32)
    one, clamp = np.float32(1.0), np.float32(1e-12)
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    a1, a0, g = np.float32(st.a1), np.float32(st.a0), st.gamma
    if mutate == 'focal_swap_alpha':
        a1, a0 = a0, a1
    if mutate == 'ce_norm_chw':
        sc_ce = sc_ce / C
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        if mutate == 'ce_no_clamp':
            lp = np.log(p32)
        else:
            lp = np.maximum(np.log(p32), np.float32(-100.0))
        lq = np.maximum(np.log1p(-p32), np.float32(-100.0))
        q32 = one - p32
        value, grads = 0.0, []
        if st.terms & CE:
            with np.errstate(invalid='ignore'):
                e = -(y32 * lp)
            value += sc_ce * float(e.astype(np.float64).sum())
            grads.append(np.float32(sc_ce) * (-y32 / np.maximum(p32, clamp)))
        if st.terms & FOCAL:
            plo, phi = _ipow32(p32, g)
            qlo, qhi = _ipow32(q32, g)
            e = -(((a1 * y32) * qhi) * lp + ((a0 * (one - y32)) * phi) * lq)
            value += sc_focal * float(e.astype(np.float64).sum())
            A, B = qhi / np.maximum(p32, clamp), phi / np.maximum(q32, clamp)
            if g > 0:
                gf = np.float32(g)
                if mutate != 'focal_no_g_term':
                    A = A - (gf * qlo) * lp
                B = (gf * plo) * lq - B
            else:
                B = -B
            grads.append(np.float32(sc_focal) * -((a1 * y32) * A + (a0 * (one - y32)) * B))
        if st.terms & DICE:
            s = float(st.smooth)
            I = (p32 * y32).astype(np.float64).sum(1)
            P, Y = p32.astype(np.float64).sum(1), y32.astype(np.float64).sum(1)
            den = P + Y + s
            num = 2.0 * I + (0.0 if mutate == 'dice_no_smooth_num' else s)
            value += sc_dice * float((1.0 - num / den).sum())
            k0 = (-2.0 * sc_dice / den).astype(np.float32)
            k1 = (sc_dice * num / (den * den)).astype(np.float32)
            if mutate == 'dice_k1_sign':
                k1 = -k1
            grads.append(k0[:, None, :] * y32 + k1[:, None, :])
        grad = grads[0].astype(np.float32)
        for x in grads[1:]:
            grad = (grad + x.astype(np.float32)).astype(np.float32)
    return np.float32(value), grad


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

def inputs(N, HW, C, head, seed):
    """(p, y) float64 (N, HW, C) of fp32-representable values.  p: the softmax over C (head 'softmax') or the sigmoid (head 'sigmoid')
    of seeded logits in +-4, with PLANTED_P written over the first and (reversed) the last places of the flattened tensor, as many as
    fit.  y: softmax head -- one-hot with one pixel in eight unlabelled (all zero); sigmoid head -- binary, one in three set.  Where
    HW >= 4 the last class of sample 0 is empty (Dice's Y = 0: D = s / (P + s))."""
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.rand(N, HW, C, generator=gen, dtype=F64) * 8.0 - 4.0)
    p = (torch.softmax(logits, -1) if head == 'softmax' else torch.sigmoid(logits)).float()
    flat = p.reshape(-1)
    k = min(flat.numel(), len(PLANTED_P))
    planted = torch.tensor(PLANTED_P, dtype=torch.float32)
    flat[:k] = planted[:k]
    if flat.numel() >= 2 * k:
        flat[flat.numel() - k:] = planted[:k].flip(0)
    if head == 'softmax':
        labels = torch.randint(0, C, (N, HW), generator=gen)
        y = F.one_hot(labels, C).float()
        y[torch.rand(N, HW, generator=gen) < 0.125] = 0.0
    else:
        y = (torch.rand(N, HW, C, generator=gen) < 1.0 / 3.0).float()
    if HW >= 4:
        y[0, :, C - 1] = 0.0
    return p.double(), y.double()


# ---- the oracle trainer ------------------------------------------------------------------------------------------------------------------

def seg_objective(loss_type, gen_img, y, seg_alpha, focal_gamma=2, focal_alpha=None, dice_smooth=1.0):
    """Trainer.loss_type's new objectives on NCHW tensors through patchgan_amd.losses: seg_alpha times the sum of the members."""
    from patchgan_amd import losses
    fn = {'ce': lambda: losses.ce_loss(y, gen_img), 'focal': lambda: losses.focal_loss(y, gen_img, focal_gamma, focal_alpha),
          'dice': lambda: losses.dice_loss(y, gen_img, dice_smooth)}
    return sum(fn[m]() for m in loss_type.split('+')) * seg_alpha


class SegOracleTrainer(OracleTrainer):
    """OracleTrainer whose segmentation term is one of the new objectives (loss_type 'ce' | 'focal' | 'dice' | a sum); the other five
    scalars and both updates are OracleTrainer's, operation for operation."""

    focal_gamma = 2
    focal_alpha = None
    dice_smooth = 1.0

    def batch(self, x, y, train=False, dropout_masks=None):
        x = x.to(self.dtype)
        y = y.to(self.dtype)
        gen_img = self.G(x, dropout_masks)
        disc_fake = self.D(torch.cat((x, gen_img), 1))
        ones = torch.ones_like(disc_fake)
        zeros = torch.zeros_like(disc_fake)
        gen_loss_seg = seg_objective(self.loss_type, gen_img, y, self.seg_alpha, self.focal_gamma, self.focal_alpha, self.dice_smooth)
        gen_loss_disc = bce(disc_fake, ones)
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
        loss_real = bce(disc_real, ones)
        loss_fake = bce(disc_fake2, zeros)
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
        self.last['seg'] = gen_loss_seg.item()
        vals = [gen_loss.item(), gen_loss.item(), gen_loss_disc.item(), loss_real.item(), loss_fake.item(), disc_loss.item()]
        return dict(zip(self.keys, vals))


def seg_oracle(gold, dtype, loss_type, focal_gamma=2, focal_alpha=None, dice_smooth=1.0, **kw):
    """SegOracleTrainer on a golden fixture's networks."""
    c = gold.cfg
    args = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=loss_type, dtype=dtype)
    args.update(kw)
    o = SegOracleTrainer(gold.weights('g0'), gold.weights('d0'), **args)
    o.focal_gamma, o.focal_alpha, o.dice_smooth = focal_gamma, focal_alpha, dice_smooth
    return o
