"""References, tolerances and case tables for the loss kernels of loss.hip and the Adam / bf16-padding kernels of optim_layout.hip
(pure CPU: torch + numpy; nothing here calls the library).

Tensors are float64 torch tensors of shape (B, HW, C) holding values representable in fp32 (B = ranks * N samples: the data-parallel
form computes each rank's N samples on its own and is held to the float64 computation over the concatenated batch).  The float64
references evaluate the definitions of include/patchgan_hip.h on the stored values; gradients are float64 autograd of the loss
expressions as oracle/patchgan_oracle.py writes them (the per-(n, c) coefficients are autograd of the same loss written as a function
of the five sums -- dL/dp = dL/dS0 * y + dL/dS2 for the Tversky term, dL/dS3 and dL/dS4 for BCE and MAE -- never a restated closed
form).  Two things are modelled in fp32 because the reference does them in fp32: the weighted-BCE weight
w = 1 - fl32(sum_hw y) / fl32(sum y) and the 1e-12 clamp of torch's binary_cross_entropy_backward.  The "plain fp32" evaluation does
every operation in straightforward fp32 torch / numpy ops with closed-form coefficients (an emulation of no particular kernel, fp64
sums where the kernels have fp64 sums); it decides whether a bound is sound, and carries the mutations the comparator must reject.

Tolerances (per element; eps32 = 2^-23 = one ulp relative, so "one rounding" is counted as eps32 although it costs at most half of
it; TINY = 2^-126, the smallest normal float: a result below it has no relative precision whether the hardware keeps or flushes it):
  sums S[n, c, k]    eps32 R_k A_k + HW 2^-52 A_k + HW TINY,  A_k = sum |term| (k = 3: sum |y lp| + |(1 - y) lq|);  R = (1, 0, 0, 4, 1):
                     y p and |p - y| are one rounding; y and p are fp32 values summed in fp64 (accumulation term only);
                     -(y lp + (1 - y) lq) is at most four per operand: 1 - y, log1pf (documented: 1 ulp, like logf), the product, the sum.
  prepare            fp64 arithmetic on fp64 sums: 2^-40 relative (N terms of (tp + 1) / denom, each below 1).
  value, coef        from the kernel's own read-back S in float64: one float rounding, eps32 |x| (+ 2^-40 |x| for the fp64 pow and
                     sums), and for weighted BCE 2 eps32 absolute on w: alpha / cnt * 2 eps32 (* sum |S3| for the value).
  end to end         the same plus the sums' tolerance propagated: sum |dL/dS| tol_S for the value, |d coef / dS| tol_S (autograd
                     Jacobian) for the Tversky coefficients; the other coefficients do not depend on S.
  gradient           Tversky  g = k0 y + k1:  2 eps32 (|k0 y| + |k1|) (product, sum) + eps32 (|k0 y| + |k1|) (coefficients) + TINY.
                     BCE      g = k0 (p - y) / max((1 - p) p, 1e-12) = k0 r:  4 eps32 |g| (p - y, 1 - p, the product, k0 (p - y), the
                              division: five half-ulps) + |r| tol_k0 + |k0| TINY / max(..) + TINY, tol_k0 = eps32 |k0| (+ the 2 eps32 of w).
                     MAE      equality with sign(p - y) * coef (the coefficient read back), sign(0) = 0: the sign of an fp32
                              difference is exact.
  Adam, one step     m' = m + (g - m)(1 - b1):  2 eps32 (|m| + (1 - b1) |g - m|) + TINY  (difference, product, sum);
                     v' = v b2 + ((1 - b2) g) g:  2 eps32 (b2 v + (1 - b2) g^2) + TINY  (three products, one sum);
                     d = sqrt(v') / sqrt_bc2 + eps:  tol_d = min(tol_v / (2 sqrt v'), sqrt tol_v) / sqrt_bc2 + 2 eps32 d  (sqrtf is
                     correctly rounded; |sqrt a - sqrt b| <= sqrt |a - b| covers v' at the floor);
                     p' = p - lr/bc1 (m' / d):  eps32 |p'| + lr/bc1 (tol_m / d + |m' / d| tol_d / d + 2 eps32 |m' / d|) + TINY:
                     relative to the update, not to the weight, except for the last rounding.
  pg_pad8_bf16       bit equality with round-to-nearest-even (normact_util.rne_bf16); a NaN stays a NaN; for an fp32 subnormal the
                     signed zero is accepted as well (the test requires the two kernel forms to agree with each other).
Inputs keep the references finite and the conditions are asserted here: the Tversky batch mean is >= 1e-3 (pow(m, gamma - 1)
diverges at a perfect prediction), sum y > 0 for weighted BCE, |g| <= 1e18 for Adam."""
from collections import namedtuple
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.normact_util import EPS32, rne_bf16, worst_ratio

F64, F32 = torch.float64, torch.float32
TINY = 2.0 ** -126
ACC = 2.0 ** -52
R_SUMS = (1.0, 0.0, 0.0, 4.0, 1.0)
MODES = ('tversky', 'wbce', 'mae', 'bce')
MODE_CODE = {'tversky': 0, 'wbce': 1, 'mae': 2, 'bce': 3}
GMODE = {'tversky': 0, 'wbce': 1, 'mae': 2, 'bce': 1}
ALPHA = {'tversky': 200.0, 'wbce': 200.0, 'mae': 200.0, 'bce': 0.5}
BETA, GAMMA = 0.75, 0.75
PLANTED_P = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 2.0 ** -149)
CLAMP = float(np.float32(1e-12))          # torch's binary_cross_entropy_backward holds its 1e-12 as a float, in float64 too


# ---- float64 references: sums ----------------------------------------------------------------------------------------------------------

def _terms(p, y):
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)
    a, b = y * lp, (1.0 - y) * lq
    return (y * p, y, p, -(a + b), (p - y).abs()), ((y * p).abs(), y.abs(), p.abs(), a.abs() + b.abs(), (p - y).abs())


def sums_ref(p, y):
    """(S, A): the five per-(n, c) sums of the header over HW, float64, (B, C, 5), and the sums of the terms' magnitudes."""
    t, a = _terms(p, y)
    S, A = torch.stack([x.sum(1) for x in t], -1), torch.stack([x.sum(1) for x in a], -1)
    assert bool(torch.isfinite(S).all())
    return S, A


def tol_sums(A, HW):
    return A * (EPS32 * torch.tensor(R_SUMS, dtype=F64) + HW * ACC) + HW * TINY


# ---- float64 references: value and coefficients as functions of S ---------------------------------------------------------------------

def tversky_acc(S, beta=BETA):
    tp = S[..., 0].sum(1)
    fn, fp = S[..., 1].sum(1) - tp, S[..., 2].sum(1) - tp
    return (1.0 - (tp + 1.0) / (tp + beta * fn + (1.0 - beta) * fp + 1.0)).sum()


def prepare_ref(S, beta=BETA):
    """pg_loss_prepare: (sum_n (1 - T_n), sum y)."""
    return torch.stack([tversky_acc(S, beta), S[..., 1].sum()])


def wbce_weight(S1, gs1, C):
    """1 - fl32(sum_hw y) / fl32(sum y), in fp32 arithmetic (ones for C == 1); float64 tensor shaped like S1."""
    if C == 1:
        return torch.ones_like(S1)
    assert float(gs1) > 0
    w = np.float32(1.0) - S1.detach().numpy().astype(np.float32) / np.float32(float(gs1))
    return torch.from_numpy(w.astype(np.float64))


def loss_of_S(mode, S, gsum2, Bglobal, HW, alpha, beta=BETA, gamma=GAMMA):
    """The loss value a rank reports, float64, differentiable in its own S ((N, C, 5)); gsum2 = the batch-global prepare terms."""
    N, C, _ = S.shape
    cnt = float(Bglobal) * C * HW
    if mode == 'tversky':
        acc = tversky_acc(S, beta)
        m = (acc + (gsum2[0] - acc).detach()) / Bglobal
        assert float(m.detach()) >= 1e-3, float(m.detach())
        return alpha * m ** gamma
    if mode == 'wbce':
        return alpha * (wbce_weight(S[..., 1], gsum2[1], C) * S[..., 3]).sum() / cnt
    return alpha * S[..., 4 if mode == 'mae' else 3].sum() / cnt


def _coef_of_S(mode, S, gsum2, Bglobal, HW, alpha, create_graph=False):
    L = loss_of_S(mode, S, gsum2, Bglobal, HW, alpha)
    dS, = torch.autograd.grad(L, S, create_graph=create_graph)
    k0 = dS[..., {'tversky': 0, 'wbce': 3, 'mae': 4, 'bce': 3}[mode]]
    k1 = dS[..., 2] if mode == 'tversky' else torch.zeros_like(k0)
    return L, torch.stack([k0, k1], -1), dS


def value_coef_ref(mode, S, gsum2, Bglobal, HW, alpha, tol_S=None):
    """(loss, coef (N, C, 2), tol_loss, tol_coef) in float64 from the sums S.  tol_S None: S is the kernel's own read-back, the result is
    one float rounding away; otherwise S is the reference's and its tolerance is propagated (end to end)."""
    N, C, _ = S.shape
    S = S.detach().clone().requires_grad_(True)
    gsum2 = gsum2.detach()
    L, coef, dS = _coef_of_S(mode, S, gsum2, Bglobal, HW, alpha)
    L, coef, dS = L.detach(), coef.detach(), dS.detach()
    tl, tc = (EPS32 + 2.0 ** -40) * L.abs(), (EPS32 + 2.0 ** -40) * coef.abs()
    if mode == 'wbce' and C > 1:
        cnt = float(Bglobal) * C * HW
        tl = tl + alpha / cnt * 2 * EPS32 * S[..., 3].detach().abs().sum()
        tc = tc + torch.tensor([alpha / cnt * 2 * EPS32, 0.0], dtype=F64)
    if tol_S is not None:
        tl = tl + (dS.abs() * tol_S).sum()
        if mode == 'tversky':
            J = torch.autograd.functional.jacobian(lambda s: _coef_of_S(mode, s, gsum2, Bglobal, HW, alpha, True)[1], S)
            tc = tc + (J.abs() * tol_S).sum((-1, -2, -3))
    assert bool(torch.isfinite(L)) and bool(torch.isfinite(coef).all())
    return L, coef, tl, tc


# ---- float64 references: gradient by autograd over the whole batch ------------------------------------------------------------------------

def loss_of_p(mode, p, y, alpha, beta=BETA, gamma=GAMMA):
    """The global loss over the concatenated batch p, y ((B, HW, C)), written like oracle.patchgan_oracle.seg_loss / bce."""
    if mode == 'tversky':
        tp, fn, fp = (y * p).sum((1, 2)), ((1.0 - p) * y).sum((1, 2)), (p * (1.0 - y)).sum((1, 2))
        tv = (tp + 1) / (tp + beta * fn + (1.0 - beta) * fp + 1)
        m = torch.mean(1 - tv)
        assert float(m.detach()) >= 1e-3, float(m.detach())
        return torch.pow(m, gamma) * alpha
    if mode == 'wbce':
        weight = wbce_weight(y.sum(1), y.sum(), p.shape[2]).unsqueeze(1).expand_as(p)
        return F.binary_cross_entropy(p, y, weight=weight) * alpha
    if mode == 'mae':
        return torch.mean(torch.abs(p - y)) * alpha
    return F.binary_cross_entropy(p, y) * alpha


def grad_ref(mode, p, y, alpha):
    q = p.detach().clone().requires_grad_(True)
    L = loss_of_p(mode, q, y, alpha)
    g, = torch.autograd.grad(L, q)
    assert bool(torch.isfinite(L)) and bool(torch.isfinite(g).all())
    return L.detach(), g


def tol_grad(mode, p, y, g, coef, tol_coef):
    """Per-element tolerance of the gradient g ((N, HW, C)) given the float64 coefficients (N, C, 2) and their tolerance."""
    k0, k1 = coef[..., 0].unsqueeze(1), coef[..., 1].unsqueeze(1)
    t0, t1 = tol_coef[..., 0].unsqueeze(1), tol_coef[..., 1].unsqueeze(1)
    if mode == 'tversky':
        return 2 * EPS32 * ((k0 * y).abs() + k1.abs()) + y.abs() * t0 + t1 + TINY
    den = ((1.0 - p) * p).clamp_min(CLAMP)
    return 4 * EPS32 * g.abs() + ((p - y) / den).abs() * t0 + k0.abs() * TINY / den + TINY


def coef_tol_for_grad(mode, coef, C, Bglobal, HW, alpha):
    """One eps32 relative for the coefficient (weighted BCE: plus the 2 eps32 absolute of w)."""
    t = EPS32 * coef.abs()
    if mode == 'wbce' and C > 1:
        t = t + torch.tensor([alpha / (float(Bglobal) * C * HW) * 2 * EPS32, 0.0], dtype=F64)
    return t


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

LossCase = namedtuple('LossCase', 'name N C H W target skew ranks nsplit kernel seed')
TARGETS = ('bin', 'frac', 'const0', 'const1')


def _lc(N, C, H, W, target='bin', skew=False, ranks=1, nsplit=1, kernel='generic', tag=None):
    name = f'{tag or ("unsplit" if nsplit == 1 else "split")}-{N}x{C}x{H}x{W}-{target}' + ('-skew' if skew else '') + ('-2ranks' if ranks == 2 else '')
    return LossCase(name, N, C, H, W, target, skew, ranks, nsplit, kernel, 1000 + 37 * N + 11 * C + H + (TARGETS.index(target) if target in TARGETS else 9))


def loss_nsplit(N, HW, C):
    """Host mirror of loss.hip's split rule (asserted against the library's own answers in the GPU tests): (nsplit, four-channel kernel)."""
    c4 = C == 4 and HW >= 4096
    ns = min(1024 // N if c4 else 256 // (N * C), HW // 1024, 128 if c4 else 64)
    ns = max(ns, 1)
    return ns, c4 and ns > 1


def reduce_cases():
    cs = [_lc(N, C, H, W, t) for C in (1, 3, 4, 7) for N in (2, 3) for H, W in ((11, 13), (20, 15)) for t in TARGETS]
    for t in TARGETS:
        cs += [_lc(2, 1, 48, 48, t, nsplit=2), _lc(2, 4, 63, 65, t, nsplit=3, tag='split-under-c4-cut'),
               _lc(3, 4, 64, 65, t, nsplit=4, kernel='c4', tag='c4')]
    return cs


# gradient layouts: (ld, off) of p, y, g; y None: the constant target.  C == 4 names the alignment mix, the others run the scalar loop.
GRAD_LAYOUTS = {
    'scalar': dict(p=(3, 1), y=(0, 0), g=(2, 1)),           # (ld - C, off)
    'vector-ld4': dict(p=(0, 0), y=(0, 0), g=(0, 0)),
    'vector-ld8off4': dict(p=(4, 4), y=(4, 4), g=(4, 4)),
    'mixed-production': dict(p=(3, 3), y=(0, 0), g=(0, 0)),
    'mixed-gslice': dict(p=(0, 0), y=(0, 0), g=(3, 3)),
    'vector-ynull': dict(p=(0, 0), y=None, g=(0, 0)),
}


def chain_cases():
    """(case, layout name) of the reduce -> prepare -> finalize -> grad chain; every one runs all four loss modes."""
    cs = [(_lc(3, C, 20, 15, 'bin' if C != 3 else 'frac', tag='chain'), 'scalar') for C in (1, 3, 7)]
    cs += [(_lc(3, 4, 20, 15, 'const1' if lay == 'vector-ynull' else 'bin', tag='chain'), lay) for lay in GRAD_LAYOUTS if lay != 'scalar']
    cs += [(_lc(2, 2, 11, 13, 'bin', skew=True, tag='chain'), 'scalar'), (_lc(2, 3, 11, 13, 'bin', ranks=2, tag='chain'), 'scalar'),
           (_lc(2, 4, 11, 13, 'frac', ranks=2, tag='chain'), 'mixed-production'),
           (_lc(3, 4, 64, 65, 'bin', nsplit=4, kernel='c4', tag='chain-c4'), 'mixed-production'),
           (_lc(2, 1, 48, 48, 'const1', nsplit=2, tag='chain-split'), 'scalar')]
    return cs


FUSED_REMAINDER = _lc(10, 1, 160, 160, 'const1', nsplit=25, tag='fused-remainder')
MULTITRIP = _lc(33, 1, 256, 256, 'const1', nsplit=7, tag='grad-multitrip')


@functools.lru_cache(maxsize=None)
def loss_inputs(case):
    """(p, y): (B, HW, C) float64 of fp32 values, B = ranks * N.  p uniform in [0, 1) with the planted values 0, 1, 2^-24, 1 - 2^-24 and
    the smallest subnormal at the start of sample 0 and at the ragged end of the last sample, and p == y on every 17th pixel of channel
    0; y binary (30 % ones), fractional, or the constant 0 / 1.  skew: y is all ones in (sample 0, channel 0), one pixel elsewhere."""
    B, HW, C = case.ranks * case.N, case.H * case.W, case.C
    gen = torch.Generator().manual_seed(case.seed)
    p = torch.rand((B, HW, C), generator=gen, dtype=F32).double()
    r = torch.rand((B, HW, C), generator=gen, dtype=F32)
    if case.target == 'bin':
        y = (r > 0.7).double()
    elif case.target == 'frac':
        y = r.double()
    else:
        y = torch.full((B, HW, C), 1.0 if case.target == 'const1' else 0.0, dtype=F64)
    if case.skew:
        y.zero_()
        y[0, :, 0] = 1.0
        y[1, 5, 1] = 1.0
    p[:, ::17, 0] = y[:, ::17, 0]
    k = len(PLANTED_P)
    plant = torch.tensor(PLANTED_P, dtype=F64)
    p[0, 1:1 + k, 0] = plant
    p[-1, HW - k:, C - 1] = plant
    if case.target == 'frac':
        p[0, 1 + k:1 + 2 * k, 0], y[0, 1 + k:1 + 2 * k, 0] = plant, torch.tensor((1.0, 0.0, 0.5, 0.25, 1.0), dtype=F64)
    assert torch.equal(p.float().double(), p) and torch.equal(y.float().double(), y)
    return p, y


def tconst_of(case):
    return {'const0': 0.0, 'const1': 1.0}.get(case.target)


@functools.lru_cache(maxsize=None)
def chain_ref(case, mode):
    """Everything the checks of one (case, mode) need, float64, over the whole batch of ranks * N samples."""
    p, y = loss_inputs(case)
    HW, alpha = case.H * case.W, ALPHA[mode]
    B = case.ranks * case.N
    S, A = sums_ref(p, y)
    if mode == 'wbce':
        assert float(S[..., 1].sum()) > 0
    L, g = grad_ref(mode, p, y, alpha)
    return dict(p=p, y=y, S=S, tol_S=tol_sums(A, HW), gsum2=prepare_ref(S), L=L, g=g, B=B, HW=HW, alpha=alpha)


def chain_ratios(case, mode, got):
    """Worst |got - ref| / tol of each check of the chain.  got: one dict per rank with S (N, C, 5) float64, sums (2,) float64 (prepare),
    coef (N, C, 2), loss (scalar), g (N, HW, C)."""
    ref = chain_ref(case, mode)
    N, C, HW, B, alpha = case.N, case.C, ref['HW'], ref['B'], ref['alpha']
    gsum2_got = sum(r['sums'].double() for r in got)
    out = {}

    def put(k, v):
        out[k] = max(out.get(k, 0.0), v)
    for rank, r in enumerate(got):
        sl = slice(rank * N, (rank + 1) * N)
        Sg = r['S'].double()
        put('sums', worst_ratio(Sg, ref['S'][sl], ref['tol_S'][sl]))
        if not bool(torch.isfinite(Sg).all()):
            continue
        want2 = prepare_ref(Sg)
        put('prepare', worst_ratio(r['sums'], want2, 2.0 ** -40 * torch.stack([torch.tensor(float(N), dtype=F64), want2[1].abs()])))
        L, coef, tl, tc = value_coef_ref(mode, Sg, gsum2_got, B, HW, alpha)
        put('value', worst_ratio(r['loss'].reshape(()), L, tl))
        put('coef', worst_ratio(r['coef'], coef, tc))
        L, coef, tl, tc = value_coef_ref(mode, ref['S'][sl], ref['gsum2'], B, HW, alpha, ref['tol_S'][sl])
        put('value_e2e', worst_ratio(r['loss'].reshape(()), L, tl))
        put('coef_e2e', worst_ratio(r['coef'], coef, tc))
        p, y, g = ref['p'][sl], ref['y'][sl], ref['g'][sl]
        if mode == 'mae':
            want = torch.sign(p - y) * r['coef'].double()[..., 0].unsqueeze(1)
            put('grad', worst_ratio(r['g'], want, torch.zeros_like(want)))
            put('grad_e2e', worst_ratio(r['g'], g, EPS32 * g.abs() + tc[..., 0].unsqueeze(1)))
        else:
            put('grad', worst_ratio(r['g'], g, tol_grad(mode, p, y, g, coef, coef_tol_for_grad(mode, coef, C, B, HW, alpha))))
    return out


# ---- plain fp32 evaluation of the chain and its mutations ---------------------------------------------------------------------------------

SUM_MUTATIONS = ('swap_channels', 'drop_tail', 'drop_slab', 'no_log_clamp')
FIN_MUTATIONS = ('w_sample0', 'w_local_sumy', 'c0_no_1mbeta', 'cnt_N')
GRAD_MUTATIONS = ('n_decode', 'stale_lane3', 'no_clamp', 'clamp_1e-6', 'sign0_is_1')


def plain_sums(p, y, mut=None, nsplit=1):
    """fp32 terms, summed in float64 like the kernels' accumulators: (N, C, 5)."""
    pf, yf = p.float(), y.float()
    lp, lq = torch.log(pf), torch.log1p(-pf)
    lp = lp.clamp_min(-100.0)
    if mut != 'no_log_clamp':
        lq = lq.clamp_min(-100.0)
    t = torch.stack([yf * pf, yf, pf, -(yf * lp + (1.0 - yf) * lq), (pf - yf).abs()], -1).double()      # (N, HW, C, 5)
    HW = t.shape[1]
    keep = torch.ones(HW, dtype=torch.bool)
    if mut == 'drop_tail':
        keep[HW - HW % 256:] = False
    if mut == 'drop_slab':
        keep[(torch.arange(HW) // 256) % nsplit == nsplit - 1] = False
    S = t[:, keep].sum(1)
    if mut == 'swap_channels':
        S = S.clone()
        S[0, [0, 1]] = S[0, [1, 0]]
    return S


def plain_prepare(S, beta=BETA):
    tp, sy, sp = S[..., 0].sum(1), S[..., 1].sum(1), S[..., 2].sum(1)
    den = tp + beta * (sy - tp) + (1.0 - beta) * (sp - tp) + 1.0
    return torch.stack([(1.0 - (tp + 1.0) / den).sum(), sy.sum()])


def plain_finalize(mode, S, gsum2, Bglobal, HW, alpha, mut=None, beta=BETA, gamma=GAMMA):
    """Closed-form value and coefficients in float64 from S, rounded once to fp32 (w in fp32): (loss, coef (N, C, 2)) as fp32."""
    N, C, _ = S.shape
    cnt = float(N if mut == 'cnt_N' else Bglobal) * C * HW
    coef = torch.zeros((N, C, 2), dtype=F64)
    if mode == 'tversky':
        m = gsum2[0] / Bglobal
        Kf = alpha * gamma * m ** (gamma - 1.0) / Bglobal
        tp, sy, sp = S[..., 0].sum(1), S[..., 1].sum(1), S[..., 2].sum(1)
        den = tp + beta * (sy - tp) + (1.0 - beta) * (sp - tp) + 1.0
        coef[..., 0] = (-Kf / den).unsqueeze(1)
        coef[..., 1] = (Kf * (tp + 1.0) * (1.0 if mut == 'c0_no_1mbeta' else 1.0 - beta) / (den * den)).unsqueeze(1)
        loss = alpha * m ** gamma
    elif mode == 'wbce':
        gs = S[..., 1].sum() if mut == 'w_local_sumy' else gsum2[1]
        w = wbce_weight(S[..., 1], gs, C)
        if mut == 'w_sample0':
            w = w[:1].expand_as(w)
        coef[..., 0] = alpha * w / cnt
        loss = alpha * (w * S[..., 3]).sum() / cnt
    else:
        coef[..., 0] = alpha / cnt
        loss = alpha * S[..., 4 if mode == 'mae' else 3].sum() / cnt
    return loss.float(), coef.float()


def plain_grad(mode, p, y, coef, mut=None):
    """The three gmodes in fp32 ops from fp32 coefficients (N, C, 2): (N, HW, C) fp32."""
    N, HW, C = p.shape
    pf, yf = p.float(), y.float()
    n = torch.arange(N * HW) // (HW + 1 if mut == 'n_decode' else HW)
    k = coef[n].view(N, HW, C, 2)
    k0, k1 = k[..., 0], k[..., 1]
    if mode == 'tversky':
        g = k0 * yf + k1
    elif mode == 'mae':
        d = pf - yf
        g = k0 * torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, 1.0 if mut == 'sign0_is_1' else 0.0)).float()
    else:
        den = (1.0 - pf) * pf
        if mut != 'no_clamp':
            den = den.clamp_min(1e-6 if mut == 'clamp_1e-6' else 1e-12)
        g = k0 * (pf - yf) / den
    if mut == 'stale_lane3':
        g = g.clone().view(N * HW, C)
        g[1:, 3] = g[:-1, 3].clone()
        g = g.view(N, HW, C)
    return g


def plain_chain(case, mode, mut=None):
    """The chain of one (case, mode) in plain fp32, one dict per rank (the shape chain_ratios takes)."""
    p, y = loss_inputs(case)
    N, HW, alpha, B = case.N, case.H * case.W, ALPHA[mode], case.ranks * case.N
    ranks = []
    for rank in range(case.ranks):
        sl = slice(rank * N, (rank + 1) * N)
        S = plain_sums(p[sl], y[sl], mut, case.nsplit)
        ranks.append(dict(S=S, sums=plain_prepare(S) if bool(torch.isfinite(S).all()) else torch.full((2,), float('nan'), dtype=F64)))
    gsum2 = sum(r['sums'] for r in ranks)
    for rank, r in enumerate(ranks):
        sl = slice(rank * N, (rank + 1) * N)
        r['loss'], r['coef'] = plain_finalize(mode, r['S'], gsum2, B, HW, alpha, mut)
        r['g'] = plain_grad(mode, p[sl], y[sl], r['coef'], mut)
    return ranks


# mutation -> (case, mode, the check that must reject it)
def mutation_table():
    by = {c.name: c for c in reduce_cases()}
    ch = {(c.name, lay): c for c, lay in chain_cases()}
    dp = ch[('chain-2x3x11x13-bin-2ranks', 'scalar')]
    c4 = ch[('chain-3x4x20x15-bin', 'vector-ld4')]
    c3 = ch[('chain-3x3x20x15-frac', 'scalar')]
    return {
        'swap_channels': (by['unsplit-2x3x11x13-bin'], 'bce', 'sums'),
        'drop_tail': (by['unsplit-3x7x20x15-frac'], 'bce', 'sums'),
        'drop_slab': (by['split-2x1x48x48-bin'], 'bce', 'sums'),
        'no_log_clamp': (by['unsplit-2x1x11x13-const0'], 'bce', 'sums'),
        'w_sample0': (c3, 'wbce', 'coef'),
        'w_local_sumy': (dp, 'wbce', 'coef'),
        'c0_no_1mbeta': (c3, 'tversky', 'coef'),
        'cnt_N': (dp, 'mae', 'coef'),
        'n_decode': (c3, 'wbce', 'grad'),
        'stale_lane3': (c4, 'tversky', 'grad'),
        'no_clamp': (c3, 'bce', 'grad'),
        'clamp_1e-6': (c3, 'bce', 'grad'),
        'sign0_is_1': (c3, 'mae', 'grad'),
    }


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------

AdamCase = namedtuple('AdamCase', 'n t lr carried')
ADAM_NS = (1, 3, 4, 5, 1023, 1024, 4099)
ADAM_BIG_N = 8388608 + 1027          # 8192 * 256 float4s fill the first grid trip: 256 float4s of a second trip, a ragged body, 3 tail elements
ADAM_FIRST_TRIP = 8192 * 256 * 4
ADAM_MUTATIONS = ('eps_in_sqrt', 'bc2_not_sqrt', 'old_m', 'v_from_abs_g', 'tail_untouched', 'second_trip_untouched')
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def adam_cases():
    return [AdamCase(n, t, lr, c) for n in ADAM_NS for t in (1, 2, 1000, 100000) for lr in (1e-3, 2e-4) for c in (False, True)]


ADAM_BIG = AdamCase(ADAM_BIG_N, 1000, 2e-4, True)


def adam_scalars(t, lr):
    """(beta1, beta2, eps, lr / bc1, sqrt(bc2)) as the float32 values the kernel receives."""
    from patchgan_amd import engine as E
    a, b = E.adam_scalars(t, lr, B1, B2)
    return tuple(float(np.float32(x)) for x in (B1, B2, ADAM_EPS, a, b))


@functools.lru_cache(maxsize=4)
def adam_inputs(case):
    """fp32 state (p, g, m, v) as float64 tensors: |g| = 10^u, u uniform in [-25, 18], random sign; carried moments: m = 0.1 randn,
    v = 10^u over [-12, -2]; g = 0 on v = 0 planted at the first, every 97th and the last element (m = 0 there when not carried)."""
    n = case.n
    gen = torch.Generator().manual_seed(4000 + n % 1000 + case.t % 7)
    p = torch.randn(n, generator=gen, dtype=F32)
    g = (10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 43 - 25)).float() * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    if case.carried:
        m = 0.1 * torch.randn(n, generator=gen, dtype=F32)
        v = (10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 10 - 12)).float()
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    for x in (g, v):
        x[::97] = 0.0
        x[-1] = 0.0
    assert float(g.abs().max()) <= 1e18 and bool((v >= 0).all())
    return tuple(x.double() for x in (p, g, m, v))


def adam_ref(state, sc):
    """One step in float64 from the fp32 state; 1 - beta formed in float32.  Returns (p', m', v') and their tolerances."""
    p, g, m, v = state
    b1, b2, eps, lrbc1, sbc2 = sc
    o1, o2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    m1 = m + (g - m) * o1
    v1 = v * b2 + o2 * g * g
    d = torch.sqrt(v1) / sbc2 + eps
    q = m1 / d
    p1 = p - lrbc1 * q
    tm = 2 * EPS32 * (m.abs() + o1 * (g - m).abs()) + TINY
    tv = 2 * EPS32 * (b2 * v + o2 * g * g) + TINY
    td = torch.minimum(tv / (2 * torch.sqrt(v1)).clamp_min(1e-300), torch.sqrt(tv)) / sbc2 + 2 * EPS32 * d
    tp = EPS32 * p1.abs() + lrbc1 * (tm / d + q.abs() * td / d + 2 * EPS32 * q.abs()) + TINY
    assert all(bool(torch.isfinite(x).all()) for x in (p1, m1, v1, tp))
    return (p1, m1, v1), (tp, tm, tv)


def plain_adam(state, sc, mut=None):
    """One step in plain fp32 torch ops."""
    p, g, m, v = (x.float() for x in state)
    b1, b2, eps, lrbc1, sbc2 = (torch.tensor(x, dtype=F32) for x in sc)
    one = torch.tensor(1.0, dtype=F32)
    m1 = m + (g - m) * (one - b1)
    v1 = v * b2 + (one - b2) * (g.abs() if mut == 'v_from_abs_g' else g * g)
    if mut == 'eps_in_sqrt':
        d = torch.sqrt(v1 + eps) / sbc2
    elif mut == 'bc2_not_sqrt':
        d = torch.sqrt(v1) / (sbc2 * sbc2) + eps
    else:
        d = torch.sqrt(v1) / sbc2 + eps
    p1 = p - lrbc1 * ((m if mut == 'old_m' else m1) / d)
    n = p.numel()
    lo = n - n % 4 if mut == 'tail_untouched' else ADAM_FIRST_TRIP if mut == 'second_trip_untouched' else n
    if lo < n:
        p1, m1, v1 = (torch.cat([a[:lo], b[lo:]]) for a, b in ((p1, p), (m1, m), (v1, v)))
    return p1, m1, v1


def adam_ratios(got, ref, tol):
    return {k: worst_ratio(a, b, t) for k, a, b, t in zip(('p', 'm', 'v'), got, ref, tol)}


def adam_mutation_table():
    return {'eps_in_sqrt': (AdamCase(1023, 1000, 1e-3, True), 'p'), 'bc2_not_sqrt': (AdamCase(1023, 2, 1e-3, True), 'p'),
            'old_m': (AdamCase(1023, 1000, 1e-3, True), 'p'), 'v_from_abs_g': (AdamCase(1023, 1000, 1e-3, True), 'v'),
            'tail_untouched': (AdamCase(4099, 1000, 1e-3, True), 'm'), 'second_trip_untouched': (ADAM_BIG, 'm')}


# ---- pg_pad8_bf16 --------------------------------------------------------------------------------------------------------------------------

# fp32 bit patterns: bf16 ties of both parities and one fp32 ulp on either side, +-0, the largest finite float, +-inf, NaN, subnormals
PAD_BITS = (0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000, 0xBF808001, 0xBF817FFF,
            0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
            0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00400000, 0x807FFFFF, 0x00008001)
PAD_CS = (1, 3, 4, 7, 8)
PAD_NPIX = (1, 255, 257)


def pad_inputs(npix, C):
    """(src bits (npix, 8) int32 with live non-zero data in every channel, expected bf16 bits (npix, 8) int32 with zero pads, subnormal
    mask, NaN mask): the special patterns cycle through the pixels' first C channels, randn fills the rest."""
    gen = torch.Generator().manual_seed(77 + npix + C)
    src = (torch.randn((npix, 8), generator=gen, dtype=F32) + 3.0).view(torch.int32).clone()
    flat = src[:, :C].reshape(-1)
    sp = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in PAD_BITS], dtype=torch.int64).to(torch.int32)
    idx = torch.arange(flat.numel())
    flat = torch.where(idx % 3 != 2, sp[(idx // 3 * 2 + idx % 3) % len(sp)], flat)
    src[:, :C] = flat.view(npix, C)
    val = src.view(F32)
    want = rne_bf16(torch.nan_to_num(val.double(), nan=0.0)).float().view(torch.int32) >> 16 & 0xFFFF
    want[:, C:] = 0
    sub = (val != 0) & (val.abs() < TINY)
    nan = torch.isnan(val)
    sub[:, C:], nan[:, C:] = False, False
    return src, want, sub, nan


def pad_mismatches(got, want, sub, nan):
    """Number of bf16 bit patterns (int32 (npix, 8), low 16 bits) that are neither the rounding, a NaN for a NaN, nor -- for an fp32
    subnormal -- the signed zero."""
    got = got & 0xFFFF
    ok = (got == want) | (nan & ((got & 0x7FFF) > 0x7F80)) | (sub & ((got & 0x7FFF) == 0) & ((got & 0x8000) == (want & 0x8000)))
    ok = torch.where(nan, (got & 0x7FFF) > 0x7F80, ok)
    return int((~ok).sum())
