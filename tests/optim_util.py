"""References, tolerances, cases and mutations for the optimizer's options: pg_adamw_step / pg_adamw_step_dev of optim_layout.hip and the
Adam entry points at betas other than (0.9, 0.999) (pure CPU: torch + numpy; nothing here calls the library).

The reference of one AdamW step is float64 from the fp32 state: p0 = p * dm, dm the float32 multiplier the kernel receives taken as a
double -- (float)(1.0 - (double)lr * weight_decay), what torch.optim.AdamW's param.mul_(1 - lr * weight_decay) multiplies by --, then
tests/lossopt_util.adam_ref on (p0, g, m, v), which test_lossopt_cpu holds to torch's own Adam step.

Tolerances (EPS32 = 2^-23; all derived):
  m, v   adam_ref's own: neither sees the decay.
  p      adam_ref's tol_p evaluated at p0, plus EPS32 |p0|: the kernel rounds the one product p * dm to fp32 (half an ulp, <= 2^-24 |p0|
         relative, inside EPS32 |p0|), and p' = p0 - u passes that error on with factor 1.
A network without a decay (dm None) is held to adam_ref as it stands."""
from collections import namedtuple
import math

import numpy as np
import torch

from tests.lossopt_util import ADAM_BIG_N, ADAM_EPS, ADAM_NS, AdamCase, F32, F64, TINY, adam_inputs, adam_ratios, adam_ref, plain_adam
from tests.normact_util import EPS32, worst_ratio

BETAS = ((0.9, 0.999), (0.5, 0.999), (0.0, 0.9))
LR_WD = ((1e-3, 1e-2), (2e-4, 0.1), (0.1, 0.5))
STEPS = (1, 2, 1000)
NEW_BETAS = BETAS[1:]
NEW_BETA_NS = (5, 1023, 4099)

OptCase = namedtuple('OptCase', 'n t lr wd b1 b2 carried')


def opt_cases(n):
    return [OptCase(n, t, lr, wd, b1, b2, c) for t in STEPS for (b1, b2) in BETAS for (lr, wd) in LR_WD for c in (False, True)]


OPT_BIG = OptCase(ADAM_BIG_N, 1000, 2e-4, 0.1, 0.5, 0.999, True)


def decay_mul(lr, wd):
    """The float32 multiplier as a Python float: formed in double, rounded once."""
    return float(np.float32(1.0 - float(lr) * float(wd)))


def scalars(t, lr, b1, b2):
    """(beta1, beta2, eps, lr / bc1, sqrt(bc2)) as the float32 values the kernel receives (lossopt_util.adam_scalars at any betas)."""
    bc1 = np.float32(1.0 - b1 ** t)
    vals = (b1, b2, ADAM_EPS, np.float32(lr) / bc1, math.sqrt(1.0 - b2 ** t))
    return tuple(float(np.float32(x)) for x in vals)


def case_state(case):
    """(fp32 state as float64 tensors, the five scalars, dm) of an OptCase."""
    state = adam_inputs(AdamCase(case.n, case.t, case.lr, case.carried))
    return state, scalars(case.t, case.lr, case.b1, case.b2), (decay_mul(case.lr, case.wd) if case.wd is not None else None)


def adamw_ref(state, sc, dm):
    """One AdamW step in float64 from the fp32 state: ((p', m', v'), (tol_p, tol_m, tol_v)).  dm None: adam_ref itself."""
    if dm is None:
        return adam_ref(state, sc)
    p, g, m, v = state
    p0 = p * dm
    (p1, m1, v1), (tp, tm, tv) = adam_ref((p0, g, m, v), sc)
    return (p1, m1, v1), (tp + EPS32 * p0.abs(), tm, tv)


def adamw_ratios(got, state, sc, dm):
    ref, tol = adamw_ref(state, sc, dm)
    return adam_ratios(got, ref, tol)


def ema_ratio(got_ema, ema, p_new, ema_c):
    """|e' - (e + (p' - e) c)| <= 2^-21 max(|e|, |p'|) with the kernel's own p' (tests/gradclip_util.py: 'ema')."""
    p1 = p_new.double()
    want = ema + (p1 - ema) * ema_c
    return worst_ratio(got_ema, want, 2.0 ** -21 * torch.maximum(ema.abs(), p1.abs()) + TINY)


# ---- plain fp32 emulation and its mutations ----------------------------------------------------------------------------------------------

MUTATIONS = ('decay_after', 'decay_lr_bc1', 'tail_not_decayed', 'm_coupled', 'v_coupled')


def plain_adamw(case, mut=None):
    """One step in plain fp32 torch ops: fl32(p * dm), then lossopt_util.plain_adam.  Mutations: the decay applied after the update;
    the multiplier formed from lr / bc1; the n % 4 tail elements not decayed; m / v computed from the coupled (L2) gradient
    g + wd * p0, a quantity that depends on the decayed parameter."""
    state, sc, dm = case_state(case)
    p, g, m, v = state
    n = p.numel()
    if mut == 'decay_lr_bc1':
        dm = float(np.float32(1.0 - sc[3] * case.wd))
    dmt = torch.tensor(dm, dtype=F32)
    p0 = p.float() * dmt
    if mut == 'tail_not_decayed':
        lo = n - n % 4
        p0 = torch.cat([p0[:lo], p.float()[lo:]])
    if mut == 'decay_after':
        p1, m1, v1 = plain_adam((p, g, m, v), sc)
        return p1 * dmt, m1, v1
    p1, m1, v1 = plain_adam((p0.double(), g, m, v), sc)
    if mut in ('m_coupled', 'v_coupled'):
        gc = (g.float() + torch.tensor(case.wd, dtype=F32) * p0).double()
        _, mc, vc = plain_adam((p0.double(), gc, m, v), sc)
        m1, v1 = (mc, v1) if mut == 'm_coupled' else (m1, vc)
    return p1, m1, v1


PLANT = dict(t=2, lr=0.1, wd=0.5, b1=0.9, b2=0.999, carried=True)          # dm = 0.95: the decay is far above one ulp


def mutation_table():
    """mutation -> (the planted OptCase, the check that must reject it)."""
    return {'decay_after': (OptCase(n=1023, **PLANT), 'p'), 'decay_lr_bc1': (OptCase(n=1023, **PLANT), 'p'),
            'tail_not_decayed': (OptCase(n=4099, **PLANT), 'p'), 'm_coupled': (OptCase(n=1023, **PLANT), 'm'),
            'v_coupled': (OptCase(n=1023, **PLANT), 'v')}
