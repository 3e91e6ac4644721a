"""Per-class weights of the segmentation objectives (Trainer.class_weights; pg_seg_loss_value_grad_w, pg_seg_label_count): float64
references, tolerances, the plain-fp32 evaluation with its mutations, NumPy's label counts and the oracle trainer.  Pure CPU: torch +
numpy, nothing here calls the library.  Everything is tests/segloss_util.py's with w_c on channel c:
  ce     value alpha / (B HW) sum_c w_c sum e_c          gradient (scale_ce w_c) de/dp
  focal  value alpha / (B C HW) sum_c w_c sum e_c        gradient (scale_focal w_c) de/dp
  dice   value alpha / (B C) sum_{n,c} w_c (1 - D[n,c])  gradient k0 y + k1, (k0, k1) = d value / d (I, P)
The weights are fp32-representable float64 numbers (what the device buffer holds).

Tolerances: the count of fp32 roundings is the unweighted one -- fl32(scale * w_c) takes the place of fl32(scale), one rounding from
double either way, and w_c enters the value and the Dice coefficients in fp64, a handful of fp64 operations more, which REL64 = 2^-40
covers as it covers the others.  So every bound is segloss_util.tolerances' formula with scale -> scale * w_c, channel by channel.  A
channel with w_c == 0 keeps only the absolute floors (TINY): its gradient must be +-0."""
import numpy as np
import torch

from tests import segloss_util as U
from tests.normact_util import EPS32
from tests.segloss_util import ACC, CE, DICE, F64, FOCAL, REL64, TINY

# distinct per channel, with a 0, a non-dyadic value and a large one; channel c takes WEIGHT_POOL[c % 8] (as fp32 numbers)
WEIGHT_POOL = (0.1, 37.5, 0.0, 1.0, 2.5, 0.75, 3.0, 0.3)


def weights_for(C):
    """C fp32-representable weights from the pool, as float64 numbers.  (One channel: 0.1 alone -- no zero.)"""
    return [float(np.float32(WEIGHT_POOL[c % len(WEIGHT_POOL)] * (1 + c // len(WEIGHT_POOL)))) for c in range(C)]


def _w(w, like):
    w = torch.as_tensor(np.asarray(w, dtype=np.float32).astype(np.float64), dtype=F64)
    assert w.numel() == like.shape[-1]
    return w


# ---- float64 references --------------------------------------------------------------------------------------------------------------

def dice_of_sums_w(S, smooth, w):
    """sum_{n,c} w_c (1 - D) as a function of the sums (N, C, 3)."""
    return (w * (1.0 - (2.0 * S[..., 0] + smooth) / (S[..., 1] + S[..., 2] + smooth))).sum()


def dice_coef_w(S, scale, smooth, w, create_graph=False):
    dS, = torch.autograd.grad(scale * dice_of_sums_w(S, smooth, w), S, create_graph=create_graph)
    return dS[..., :2]


def reference(p, y, st, w):
    """{'value': float, 'grad': (N, HW, C), 'members': {name: (value, grad)}} in float64, with per-class weights w."""
    N, HW, C = p.shape
    w = _w(w, p)
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    out = {}
    if st.terms & CE:
        out['ce'] = (sc_ce * (w * U.ce_elem(p, y)).sum(), sc_ce * w * U.ce_dedp(p, y))
    if st.terms & FOCAL:
        out['focal'] = (sc_focal * (w * U.focal_elem(p, y, st)).sum(), sc_focal * w * U.focal_dedp(p, y, st))
    if st.terms & DICE:
        S = U.dice_sums(p, y).requires_grad_(True)
        k = dice_coef_w(S, sc_dice, st.smooth, w).detach()
        out['dice'] = (sc_dice * dice_of_sums_w(S.detach(), st.smooth, w), k[..., 0].unsqueeze(1) * y + k[..., 1].unsqueeze(1))
    value, grad = sum(v for v, _ in out.values()), sum(g for _, g in out.values())
    assert bool(torch.isfinite(value)) and bool(torch.isfinite(grad).all()), 'the inputs must keep the references finite'
    return {'value': float(value), 'grad': grad, 'members': out}


def loss_of_p(p, y, st, w):
    """The weighted value as a differentiable float64 expression of p."""
    N, HW, C = p.shape
    w = _w(w, p)
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    v = 0.0
    if st.terms & CE:
        v = v + sc_ce * (w * U.ce_elem(p, y)).sum()
    if st.terms & FOCAL:
        v = v + sc_focal * (w * U.focal_elem(p, y, st)).sum()
    if st.terms & DICE:
        v = v + sc_dice * dice_of_sums_w(U.dice_sums(p, y), st.smooth, w)
    return v


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------

def tolerances(p, y, st, w):
    """(tol_value, tol_grad (N, HW, C)): segloss_util.tolerances with scale -> scale * w_c on channel c."""
    N, HW, C = p.shape
    n = N * HW * C
    w = _w(w, p)
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    g = st.gamma
    tol_v, mag_v = 0.0, 0.0
    tol_g, mag_g, members = torch.zeros_like(p), torch.zeros_like(p), 0
    if st.terms & CE:
        s = sc_ce * w
        e, gr = U.ce_elem(p, y), s * U.ce_dedp(p, y)
        tol_v += float((s * (2 * EPS32 * e.abs() + TINY)).sum() + n * ACC * (s * e.abs()).sum())
        mag_v += float((s * e.abs()).sum())
        tol_g, mag_g, members = tol_g + 3 * EPS32 * gr.abs() + TINY, mag_g + gr.abs(), members + 1
    if st.terms & FOCAL:
        s = (sc_focal * w).abs()
        t1, t0 = U.focal_parts(p, y, st)
        tol_e = EPS32 * ((5 + 2 * g) * t1.abs() + (6 + g) * t0.abs()) + 2 ** 8 * TINY
        mag = t1.abs() + t0.abs()
        tol_v += float((s * tol_e).sum() + n * ACC * (s * mag).sum())
        mag_v += float((s * mag).sum())
        A1, A2, B1, B2 = U.focal_grad_parts(p, y, st)
        w1, w0 = (st.a1 * y).abs(), (st.a0 * (1.0 - y)).abs()
        tol_A, tol_B = (2 * g + 1) * EPS32 * (A1.abs() + A2.abs()), (g + 2) * EPS32 * (B1.abs() + B2.abs())
        u1, u0 = w1 * (A1 - A2).abs(), w0 * (B2 - B1).abs()
        tol_g = tol_g + s * (w1 * tol_A + w0 * tol_B + 5 * EPS32 * u1 + 6 * EPS32 * u0) + 2 ** 10 * TINY * s.clamp_min(1.0)
        mag_g, members = mag_g + s * (u1 + u0), members + 1
    if st.terms & DICE:
        S = U.dice_sums(p, y).requires_grad_(True)
        py = (p * y).abs().sum(1)
        tol_S = torch.stack([EPS32 * py + HW * ACC * py + HW * TINY, HW * ACC * S[..., 1].detach().abs(), HW * ACC * S[..., 2].detach().abs()], -1)
        val = sc_dice * dice_of_sums_w(S, st.smooth, w)
        dS, = torch.autograd.grad(val, S)
        vabs = abs(sc_dice) * float((w * (1.0 - (2.0 * S[..., 0] + st.smooth) / (S[..., 1] + S[..., 2] + st.smooth)).abs()).sum().detach())
        tol_v += float((dS.abs() * tol_S).sum()) + REL64 * vabs
        mag_v += vabs
        k = dice_coef_w(S, sc_dice, st.smooth, w).detach()
        J = torch.autograd.functional.jacobian(lambda s: dice_coef_w(s, sc_dice, st.smooth, w, True), S.detach().clone().requires_grad_(True))
        tol_k = (EPS32 + REL64) * k.abs() + (J.abs() * tol_S).sum((-1, -2, -3))
        k0y, k1 = (k[..., 0].unsqueeze(1) * y).abs(), k[..., 1].unsqueeze(1).abs().expand_as(p)
        tol_g = tol_g + 2 * EPS32 * (k0y + k1) + y.abs() * tol_k[..., 0].unsqueeze(1) + tol_k[..., 1].unsqueeze(1) + TINY
        mag_g, members = mag_g + k0y + k1, members + 1
    tol_v += (EPS32 + REL64) * mag_v + TINY
    tol_g = tol_g + (members - 1) * EPS32 * mag_g + TINY
    return float(tol_v), tol_g


class Expect:
    """The weighted float64 reference and its tolerances, computed once and shared by every call held to them."""

    def __init__(self, p, y, st, w):
        self.shape, self.ref = tuple(p.shape), reference(p, y, st, w)
        self.tol_v, self.tol_g = tolerances(p, y, st, w)

    def ratios(self, value, grad):
        """(value ratio, worst gradient ratio) in units of the bound: <= 1.0 passes, a NaN counts as inf."""
        rv = abs(float(value) - self.ref['value']) / self.tol_v
        rv = float('inf') if rv != rv else rv
        if grad is None:
            return rv, 0.0
        got = torch.as_tensor(np.asarray(grad), dtype=F64).reshape(self.shape)
        r = (got - self.ref['grad']).abs() / self.tol_g
        r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
        return rv, float(r.max())


# ---- the plain fp32 evaluation, with the mutations the comparator must reject -------------------------------------------------------

MUTATIONS = ('swap_weights', 'weight_missing_in_member', 'weight_twice')


def plain_fp32(p, y, st, w, mutate=None):
    """segloss_util.plain_fp32 with the weights as the header states them: fl32(scale * w_c) in place of fl32(scale), w_c in fp64 in
    the value and the Dice coefficients.  Mutations: 'swap_weights' -- the weights of the first two channels whose weights differ
    are exchanged; 'weight_missing_in_member' -- the LAST member of the sum is evaluated without weights; 'weight_twice' -- w_c^2."""
    N, HW, C = p.shape
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    if mutate == 'swap_weights':
        i, j = next((i, j) for i in range(C) for j in range(i + 1, C) if w64[i] != w64[j])
        w64 = w64.copy()
        w64[i], w64[j] = w64[j], w64[i]
    if mutate == 'weight_twice':
        w64 = w64 * w64
    members = st.members()
    wm = {m: (np.ones(C) if (mutate == 'weight_missing_in_member' and m == members[-1]) else w64) for m in members}
    p32, y32 = p.numpy().astype(np.float32), y.numpy().astype(np.float32)
    one, clamp = np.float32(1.0), np.float32(1e-12)
    sc_ce, sc_focal, sc_dice = st.scales(N, HW, C)
    a1, a0, g = np.float32(st.a1), np.float32(st.a0), st.gamma
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        lp = np.maximum(np.log(p32), np.float32(-100.0))
        lq = np.maximum(np.log1p(-p32), np.float32(-100.0))
        q32 = one - p32
        value, grads = 0.0, []
        if st.terms & CE:
            e = -(y32 * lp)
            value += sc_ce * float((wm['ce'] * e.astype(np.float64).sum((0, 1))).sum())
            grads.append((sc_ce * wm['ce']).astype(np.float32) * (-y32 / np.maximum(p32, clamp)))
        if st.terms & FOCAL:
            plo, phi = U._ipow32(p32, g)
            qlo, qhi = U._ipow32(q32, g)
            e = -(((a1 * y32) * qhi) * lp + ((a0 * (one - y32)) * phi) * lq)
            value += sc_focal * float((wm['focal'] * e.astype(np.float64).sum((0, 1))).sum())
            A, B = qhi / np.maximum(p32, clamp), phi / np.maximum(q32, clamp)
            if g > 0:
                gf = np.float32(g)
                A = A - (gf * qlo) * lp
                B = (gf * plo) * lq - B
            else:
                B = -B
            grads.append((sc_focal * wm['focal']).astype(np.float32) * -((a1 * y32) * A + (a0 * (one - y32)) * B))
        if st.terms & DICE:
            s = float(st.smooth)
            I = (p32 * y32).astype(np.float64).sum(1)
            P, Y = p32.astype(np.float64).sum(1), y32.astype(np.float64).sum(1)
            den = P + Y + s
            num = 2.0 * I + s
            value += sc_dice * float((wm['dice'] * (1.0 - num / den)).sum())
            sd = sc_dice * wm['dice']
            k0 = (-2.0 * sd / den).astype(np.float32)
            k1 = (sd * num / (den * den)).astype(np.float32)
            grads.append(k0[:, None, :] * y32 + k1[:, None, :])
        grad = grads[0].astype(np.float32)
        for x in grads[1:]:
            grad = (grad + x.astype(np.float32)).astype(np.float32)
    return np.float32(value), grad


# ---- label counts ------------------------------------------------------------------------------------------------------------------------

def label_counts(y):
    """pg_seg_label_count's C + 2 words for a target (N, HW, C) (any float array): NumPy's counts."""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        hit = y >= np.float32(0.5)
    C = y.shape[-1]
    per = hit.reshape(-1, C).sum(0).astype(np.int64)
    return np.concatenate([per, [int((~hit.any(-1)).sum()), int(hit.reshape(-1, C).shape[0])]]).astype(np.int64)


def count_target(N, HW, C, seed):
    """A target for the count tests: one-hot pixels, unlabelled pixels, soft and multi-hot pixels, values exactly 0.5, just below it,
    and NaNs (a NaN is not >= 0.5)."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.nn.functional.one_hot(torch.randint(0, C, (N, HW), generator=gen), C).float()
    kind = torch.rand(N, HW, generator=gen)
    y[kind < 0.125] = 0.0
    soft = torch.rand(N, HW, C, generator=gen)
    y = torch.where((kind >= 0.125).unsqueeze(-1) & (kind < 0.25).unsqueeze(-1), soft, y)
    flat = y.reshape(-1)
    planted = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), float('nan'), 1.0, 0.0, float('nan'), 0.5])
    k = min(flat.numel(), planted.numel())
    flat[:k] = planted[:k]
    if flat.numel() >= 2 * k:
        flat[flat.numel() - k:] = planted[:k].flip(0)
    return y


# ---- the oracle trainer ------------------------------------------------------------------------------------------------------------------

def seg_objective(loss_type, gen_img, y, seg_alpha, focal_gamma=2, focal_alpha=None, dice_smooth=1.0, class_weights=None):
    """segloss_util.seg_objective with class_weights passed to the torch ops of patchgan_amd.losses."""
    from patchgan_amd import losses
    fn = {'ce': lambda: losses.ce_loss(y, gen_img, class_weights=class_weights),
          'focal': lambda: losses.focal_loss(y, gen_img, focal_gamma, focal_alpha, class_weights=class_weights),
          'dice': lambda: losses.dice_loss(y, gen_img, dice_smooth, class_weights=class_weights)}
    return sum(fn[m]() for m in loss_type.split('+')) * seg_alpha


class WeightedSegOracleTrainer(U.SegOracleTrainer):
    """SegOracleTrainer whose segmentation term takes class_weights; everything else is SegOracleTrainer.batch, operation for
    operation."""

    class_weights = None

    def batch(self, x, y, train=False, dropout_masks=None):
        from oracle.patchgan_oracle import adam_update, bce
        x = x.to(self.dtype)
        y = y.to(self.dtype)
        gen_img = self.G(x, dropout_masks)
        disc_fake = self.D(torch.cat((x, gen_img), 1))
        ones = torch.ones_like(disc_fake)
        zeros = torch.zeros_like(disc_fake)
        gen_loss_seg = seg_objective(self.loss_type, gen_img, y, self.seg_alpha, self.focal_gamma, self.focal_alpha, self.dice_smooth,
                                     self.class_weights)
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


def seg_oracle(gold, dtype, loss_type, class_weights, focal_gamma=2, focal_alpha=None, dice_smooth=1.0, weights=None, **kw):
    """WeightedSegOracleTrainer on a golden fixture's networks (`weights`: (generator, discriminator) state dicts instead of the
    fixture's own, for another width)."""
    c = gold.cfg
    args = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=loss_type, dtype=dtype)
    args.update(kw)
    gw, dw = weights if weights is not None else (gold.weights('g0'), gold.weights('d0'))
    o = WeightedSegOracleTrainer(gw, dw, **args)
    o.focal_gamma, o.focal_alpha, o.dice_smooth, o.class_weights = focal_gamma, focal_alpha, dice_smooth, class_weights
    return o
