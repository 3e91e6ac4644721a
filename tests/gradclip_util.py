"""References, tolerances, cases and mutations for gradient-norm clipping: pg_grad_norm and pg_adam_clip_step / pg_adam_clip_step_dev
of optim_layout.hip (pure CPU: torch + numpy; nothing here calls the library).

The reference is torch in float64: torch.nn.utils.clip_grad_norm_ followed by Adam (tests/lossopt_util.adam_ref, which
test_lossopt_cpu holds to torch's own step) on float64 copies of the fp32 state, plus the one rule the feature adds: a step whose
float64 norm is not finite leaves the state unchanged.

Tolerances (eps32 = 2^-23, ACC = 2^-52; all derived):
  sumsq   n ACC sumsq: the squares of fp32 values are exact in fp64, and any order of summing n non-negative fp64 terms is within
          (n - 1) 2^-53 of the exact sum, relative.  (The reference's own torch.sum is pairwise: log2(n) 2^-53.)
  norm    the stored float: (n ACC + eps32) norm  (sqrt halves the sum's relative error; the correctly rounded fp64 sqrt and the one
          float rounding are inside eps32).
  coef    from the kernel's OWN read-back norm r (a float): min(1, max_norm / (r + 1e-6)), (eps32 + 2^-40) relative -- the kernel
          divides by the fp64 norm, which differs from r by 2^-24 relative, and rounds the quotient once, 2^-24.  Exactly 1 where
          r + 1e-6 <= max_norm (1 - eps32): then the fp64 quotient is >= 1 whatever the rounding of r.  (torch's 1e-6 makes the
          coefficient max_norm / (max_norm + 1e-6) < 1 AT norm == max_norm; the margin is that of the one float rounding of r.)
  update  g' = fl32(g * coef read back) taken as the fp32 gradient, then lossopt_util.adam_ref and its tolerances, unchanged.
  ema     |e' - (e + (p' - e) c)| <= 2^-21 max(|e|, |p'|), p' and c the kernel's own (tests/test_ema_gpu.py, test A).
  skip    bit equality of p, m, v (ema) with the state before, coef == 0, apply == 0.
The partition constants mirror optim_layout.hip and are asserted against pg_grad_norm_workspace_bytes in the tests that load it."""
from collections import namedtuple
import functools
import math

import numpy as np
import torch

from tests.lossopt_util import (ACC, ADAM_BIG, ADAM_BIG_N, ADAM_MUTATIONS, ADAM_NS, AdamCase, F32, F64, adam_inputs, adam_mutation_table,
                                adam_ratios, adam_ref, adam_scalars, plain_adam)
from tests.normact_util import EPS32, worst_ratio

INF = float('inf')
NORM_THREADS, NORM_MAX_BLOCKS = 256, 2048
CHUNK = NORM_THREADS * 4                      # floats one workgroup takes per grid trip
TRIP = NORM_MAX_BLOCKS * CHUNK                # floats of one trip of the full grid
STAT = np.dtype([('norm', '<f4'), ('coef', '<f4'), ('apply', '<u4'), ('reserved', '<u4'), ('steps', '<u8'), ('clipped', '<u8'),
                 ('skipped', '<u8'), ('max_norm', '<f8'), ('sum_norm', '<f8'), ('sumsq', '<f8')])


def norm_blocks(n):
    """Workgroups of pg_grad_norm's first launch (host mirror; pg_grad_norm_workspace_bytes(n) == 8 * norm_blocks(n))."""
    return max(1, min(((n >> 2) + NORM_THREADS - 1) // NORM_THREADS, NORM_MAX_BLOCKS))


# n on both sides of every boundary of the partition: the tail (n % 4), the workgroup chunk (1024 floats: one / two workgroups), the
# grid trip (2048 workgroups: one / two trips), each with and without a tail
NORM_NS = tuple(sorted(set(ADAM_NS + (CHUNK - 4, CHUNK + 1, CHUNK + 4, CHUNK + 5, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1,
                                      TRIP - CHUNK - 3, TRIP - 1, TRIP, TRIP + 1, TRIP + 4, TRIP + 5, TRIP + CHUNK + 3))))
KINDS = ('wide', 'unit', 'small', 'huge')
T_LR = (1000, 1e-3)


@functools.lru_cache(maxsize=4)
def _unit(n):
    gen = torch.Generator().manual_seed(9000 + n % 1000)
    mag = 0.5 + 1.5 * torch.rand(n, generator=gen, dtype=F32)
    return mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)


def clip_inputs(n, kind):
    """fp32 state (p, g, m, v) as float64 tensors.  p, m, v: lossopt_util.adam_inputs (carried moments).  g by kind:
    wide   adam_inputs' own: |g| = 10^u over [-25, 18], zeros planted
    unit   |g| uniform in [0.5, 2): every element carries weight in the norm (a dropped tail or trip shows)
    small  1e-4 * unit: the norm is small enough for torch's 1e-6 to matter
    huge   |g| = 10^u over [20, 30]: an fp32 sum of squares is inf, the norm is a float"""
    p, g, m, v = adam_inputs(AdamCase(n, T_LR[0], T_LR[1], True))
    if kind == 'unit':
        g = _unit(n).double()
    elif kind == 'small':
        g = (_unit(n) * 1e-4).double()
    elif kind == 'huge':
        gen = torch.Generator().manual_seed(9100 + n % 1000)
        g = ((10.0 ** (20 + 10 * torch.rand(n, generator=gen, dtype=F64))).float() * torch.sign(_unit(n))).double()
        assert float(g.abs().min()) >= 1e20
    else:
        assert kind == 'wide'
    assert torch.equal(g.float().double(), g)
    return p, g, m, v


def poisoned(state, where, value):
    """The state with one non-finite gradient element: where = 'first' | 'tail' (the last element; n % 4 != 0) | 'trip2' (the first
    element of the second grid trip; n > TRIP)."""
    p, g, m, v = state
    n = g.numel()
    i = {'first': 0, 'tail': n - 1, 'trip2': TRIP}[where]
    assert i < n and (where != 'tail' or n % 4)
    g = g.clone()
    g[i] = value
    return p, g, m, v


def sumsq_ref(g):
    return float((g * g).sum())


def norm_ref(g):
    """The float64 2-norm of the fp32 gradient: what clip_grad_norm_ computes on the float64 copy."""
    return math.sqrt(sumsq_ref(g))


def coef_ref(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def scaled(g, coef):
    """fl32(g * coef) as float64: the one fp32 product torch's grad.mul_(coef) stores."""
    return (g.float() * torch.tensor(coef, dtype=F32)).double()


def _bits_equal(a, b):
    return torch.equal(a.float().contiguous().view(torch.int32), b.float().contiguous().view(torch.int32))


def clip_ratios(got, state, sc, max_norm, ema=None, ema_c=None, norm_of=None):
    """Worst |got - ref| / tol of each check.  got: dict(sumsq, norm, coef, apply: Python numbers from the status block; p, m, v
    [, ema]: tensors).  state: the fp32 state before, float64; ema: the average before (or None), ema_c = 1 - decay as formed in fp32.
    norm_of: the float64 tensors the reference norm is taken over (a network's parameter gradients) instead of the whole of g."""
    p, g, m, v = state
    n = g.numel() if norm_of is None else sum(x.numel() for x in norm_of)
    ss = sumsq_ref(g) if norm_of is None else float(sum((x * x).sum() for x in norm_of))
    before = dict(p=p, m=m, v=v)
    if ema is not None:
        before['ema'] = ema
    if not math.isfinite(ss):
        same = all(_bits_equal(got[k], before[k]) for k in before)
        return {'skip': 0.0 if (same and got['coef'] == 0.0 and got['apply'] == 0) else INF}
    one = torch.ones((), dtype=F64)
    out = {'skip': 0.0 if got['apply'] == 1 else INF}
    out['sumsq'] = worst_ratio(one * got['sumsq'], one * ss, one * (n * ACC * ss))
    norm = math.sqrt(ss)
    out['norm'] = worst_ratio(one * got['norm'], one * norm, one * ((n * ACC + EPS32) * norm))
    r = float(got['norm'])
    if not (math.isfinite(r) and r >= 0.0):
        out['coef'] = INF
        return out
    c = coef_ref(r, max_norm)
    out['coef'] = worst_ratio(one * got['coef'], one * c, one * ((EPS32 + 2.0 ** -40) * c))
    if r + 1e-6 <= max_norm * (1.0 - EPS32) and got['coef'] != 1.0:
        out['coef'] = INF
    if not (0.0 <= got['coef'] <= 1.0):
        out['coef'] = INF
        return out
    ref, tol = adam_ref((p, scaled(g, got['coef']), m, v), sc)
    out.update(adam_ratios((got['p'], got['m'], got['v']), ref, tol))
    if ema is not None:
        p1 = got['p'].double()
        want = ema + (p1 - ema) * ema_c
        out['ema'] = worst_ratio(got['ema'], want, 2.0 ** -21 * torch.maximum(ema.abs(), p1.abs()))
    return out


# ---- plain fp32 emulation and its mutations ----------------------------------------------------------------------------------------------

NORM_MUTATIONS = ('norm_drop_tail', 'norm_drop_trip2', 'norm_fp32_acc', 'coef_no_clamp', 'coef_no_1e-6', 'coef_m_not_v', 'skip_writes_m')


def plain_clip(state, sc, max_norm, mut=None, ema=None, ema_c=None):
    """Norm, coefficient and one clipped step in plain torch / numpy ops: fp32 squares widened to fp64 and summed there, the
    coefficient in double rounded once, the fp32 product g * coef, then lossopt_util.plain_adam (which carries ADAM_MUTATIONS)."""
    p, g, m, v = state
    n = g.numel()
    gs = g
    if mut == 'norm_drop_tail':
        gs = g[:n - n % 4]
    elif mut == 'norm_drop_trip2':
        gs = g[:TRIP]
    if mut == 'norm_fp32_acc':
        with np.errstate(over='ignore'):
            gf = gs.float().numpy()
            ss = float(np.sum(gf * gf, dtype=np.float32))
    else:
        ss = float((gs * gs).sum())
    out = dict(sumsq=ss, norm=float(np.float32(math.sqrt(ss))) if ss == ss else float('nan'))
    keep = dict(p=p.float(), m=m.float(), v=v.float())
    if ema is not None:
        keep['ema'] = ema.float()
    if not math.isfinite(ss):
        out.update(coef=0.0, apply=0, **keep)
        if mut == 'skip_writes_m':
            out['m'] = plain_adam(state, sc)[1]
        return out
    c = max_norm / (math.sqrt(ss) + (0.0 if mut == 'coef_no_1e-6' else 1e-6))
    coef = float(np.float32(c if mut == 'coef_no_clamp' else min(1.0, c)))
    out.update(coef=coef, apply=1)
    amut = mut if mut in ADAM_MUTATIONS else None
    p1, m1, v1 = plain_adam((p, scaled(g, coef), m, v), sc, amut)
    if mut == 'coef_m_not_v':
        v1 = plain_adam((p, g, m, v), sc)[2]
    out.update(p=p1, m=m1, v=v1)
    if ema is not None:
        e = ema.float()
        out['ema'] = e + (p1 - e) * torch.tensor(ema_c, dtype=F32)
    return out


ClipCase = namedtuple('ClipCase', 'n kind clip')          # clip: 'below' (max_norm = norm / 4: clips) | 'above' (4 norm) | 'inf'


def max_norm_of(case, state):
    """(A 'huge' gradient is only ever clipped, and to 1: unclipped or at a quarter of its norm, Adam's own fp32 g * g overflows, with
    or without this feature.)"""
    nr = norm_ref(state[1])
    if case.kind == 'huge':
        assert case.clip == 'below'
        return 1.0
    if nr == 0.0:          # (n = 1 of 'wide' is the planted zero: nothing to clip, any max-norm gives coef == 1)
        return INF if case.clip == 'inf' else 1.0
    return {'below': nr / 4, 'above': nr * 4, 'inf': INF}[case.clip]


SMALL_NS = tuple(n for n in NORM_NS if n <= 2 * CHUNK + 1)
BIG_NS = tuple(n for n in NORM_NS if n > 2 * CHUNK + 1)


def clip_cases():
    """Every small n with every kind and every max-norm; the sizes around the grid trip with 'unit' and 'wide' gradients, clipping."""
    cs = [ClipCase(n, k, c) for n in SMALL_NS for k in KINDS for c in ('below', 'above', 'inf') if not (k == 'huge' and c != 'below')]
    cs += [ClipCase(n, k, 'below') for n in BIG_NS for k in ('unit', 'wide')]
    return cs


BIG_CASE = ClipCase(ADAM_BIG_N, 'unit', 'below')
POISON_N = TRIP + CHUNK + 3
POISONS = [(where, value) for where in ('first', 'tail', 'trip2') for value in (float('nan'), INF)]


def clip_mutation_table():
    """mutation -> (ClipCase or (ClipCase, where, value) for a poisoned one, the check that must reject it)."""
    t = {
        'norm_drop_tail': (ClipCase(4099, 'unit', 'below'), 'sumsq'),
        'norm_drop_trip2': (ClipCase(TRIP + 5, 'unit', 'below'), 'sumsq'),
        'norm_fp32_acc': (ClipCase(4099, 'huge', 'below'), 'sumsq'),
        'coef_no_clamp': (ClipCase(1023, 'wide', 'above'), 'coef'),
        'coef_no_1e-6': (ClipCase(1023, 'small', 'below'), 'coef'),
        'coef_m_not_v': (ClipCase(1023, 'unit', 'below'), 'v'),
        'skip_writes_m': ((ClipCase(4099, 'unit', 'below'), 'tail', float('nan')), 'skip'),
    }
    for mut, (acase, key) in adam_mutation_table().items():
        t[mut] = (ClipCase(acase.n, 'unit' if acase.n == ADAM_BIG.n else 'wide', 'below'), key)
    return t


def case_state(case):
    """(state, scalars, max_norm) of a ClipCase or a poisoned (ClipCase, where, value)."""
    poison = None
    if not isinstance(case, ClipCase):
        case, *poison = case
    state = clip_inputs(case.n, case.kind)
    mx = max_norm_of(case, state)
    if poison:
        state = poisoned(state, *poison)
    return state, adam_scalars(*T_LR), mx
