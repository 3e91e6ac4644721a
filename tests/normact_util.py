"""References, tolerances and case tables for the InstanceNorm / activation / softmax kernels of norm_act.hip (pure CPU: torch + numpy).

Everything here is independent of the library: the dropout mask is a NumPy port of pg_dropout_keep, the float64 references evaluate
the formulas of include/patchgan_hip.h on the stored input values, and the "plain fp32" evaluation does the same in straightforward
fp32 torch ops (an emulation of no particular kernel: it shows what a correct fp32 implementation costs, and carries the mutations
the comparator must reject).  Tensors are float64 torch tensors of shape (N, HW, C) -- element (n, pix, c) has dropout index
(n*HW + pix)*C + c -- holding values representable in the storage type of the tensor they are loaded into.

Tolerances (per element, never a global maximum; eps32 = 2^-23, ks = 1/(1-p)):
  norm forward    4 * A,  A = eps32 * (|ref| + ks * (|y| + |mean|) * rstd): the three roundings of z = y*rstd + (-mean*rstd) with fp32
                  mean and rstd are at most 3 eps32 of (|y| + |mean|) * rstd; activation and keep scale add a few ulp of the result.
  norm backward   8 * (A_b + E),  A_b = eps32 * rstd * (|dz| + |mean(dz)| + (|y - mean| + |mean|) * |kk| + |dy| / rstd);  E = the
                  largest |plain fp32 - ref| of the element's (n, c) plane: the backward is ill-conditioned exactly where any fp32
                  evaluation loses digits (mean^2 >> var), and E is measured from the independent evaluation, never from the library.
  stats           |mean - mean64| <= eps32 |mean64|;  rstd relative error <= 2 eps32 + 2^-48 (1 + mean^2 / (var + eps)) (the second
                  term: E[x^2] - mean^2 in fp64 on the chunked path).
  act forward     4 eps32 |ref| + 1e-37: activation (<= 2.5 ulp for tanhf / expf and the division), the fp32 keep scale and the
                  product, half an ulp each; 1e-37 where the result leaves the normal range (sigmoid(-90)).
  act backward    8 eps32 ks |g| (|act'| + s) + 1e-37 |g|,  s = a^2 (tanh), a (sigmoid), 0 otherwise: the un-scaled output a (1 - p)
                  carries an ulp, which 1 - a^2 and a (1 - a) turn into an absolute error of that size.
  softmax         forward eps32 (4 + |y - max|) ref + 1e-37;  backward (8 eps32 o + 1e-37) (|g| + sum_c |g_c o_c|).  The 1e-37 of the
                  backward is the forward's: an output below the normal range (exp(-89) next to a planted +80) has no relative
                  precision in fp32, stored or multiplied; without it the plain fp32 evaluation itself misses by 3.5e3.
A bf16-stored result must lie in [rne_bf16(ref - tol), rne_bf16(ref + tol)]: rounding is monotone, so that is exactly "some value
within tol of the reference rounds to what was stored"."""
from collections import namedtuple

import numpy as np
import torch

EPS32 = 2.0 ** -23
EPS = float(np.float32(1e-5))          # the kernels take eps as a float
ACTS = ('none', 'leaky', 'relu', 'tanh', 'sigmoid')
ACT_CODE = {a: i for i, a in enumerate(ACTS)}
ORACLE_ACT = {'none': None, 'leaky': 'leakyrelu', 'relu': 'relu', 'tanh': 'tanh', 'sigmoid': 'sigmoid'}
SEEDS = (0xABCDEF12345, 1, 2 ** 63 + 5)
F64, F32 = torch.float64, torch.float32


# ---- dropout mask ------------------------------------------------------------------------------------------------------------------

def keep_mask(seed, n_elems, p, start=0):
    """pg_dropout_keep(seed, e, p) for e = start .. start + n_elems - 1 as a bool array: 64-bit mix of seed + golden * (e + 1), its top
    24 bits converted to float32, times 2^-24, compared >= float32(p).  uint64 array arithmetic wraps like the device's."""
    with np.errstate(over='ignore'):
        e = np.arange(start, start + n_elems, dtype=np.uint64)
        x = np.full(1, seed % 2 ** 64, dtype=np.uint64) + np.uint64(0x9e3779b97f4a7c15) * (e + np.uint64(1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94d049bb133111eb)
        x ^= x >> np.uint64(31)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def mask_t(seed, shape, p, start=0):
    """The keep mask of an (N, HW, C) / (npix, C) tensor as float64 ones and zeros; all ones for p == 0."""
    n = int(np.prod(shape))
    if p == 0:
        return torch.ones(shape, dtype=F64)
    return torch.from_numpy(keep_mask(seed, n, p, start).astype(np.float64)).view(shape)


def keep_scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


# ---- storage types -----------------------------------------------------------------------------------------------------------------

def to_bf(x):
    """float64 -> nearest bf16-representable float64 (inputs: random values, no ties to speak of)."""
    return x.float().bfloat16().double()


def rne_bf16(x):
    """Round-to-nearest-even of float64 values to bf16, as float64, without the double rounding of float64 -> fp32 -> bf16: where the
    fp32 value lands exactly on a bf16 tie, the residual of the first rounding decides."""
    x = x.contiguous()
    f = x.float()
    r = (x - f.double()).reshape(-1).numpy()
    b = f.reshape(-1).numpy().view(np.uint32).astype(np.int64)
    low, up = b & 0xFFFF, b & ~np.int64(0xFFFF)
    odd = (b >> 16) & 1
    sgn = np.where((b >> 31) & 1 == 1, -1.0, 1.0)
    away = r * sgn                                   # > 0: the true value lies further from zero than the fp32 one
    tie = low == 0x8000
    round_up = (low > 0x8000) | (tie & (away > 0)) | (tie & (away == 0) & (odd == 1))
    out = (up + np.where(round_up, 0x10000, 0)).astype(np.uint32).view(np.float32)
    return torch.from_numpy(out.astype(np.float64)).view(x.shape)


# ---- activations -------------------------------------------------------------------------------------------------------------------

def act_f(z, act):
    if act == 'leaky':
        return torch.where(z > 0, z, z * 0.2)
    if act == 'relu':
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == 'tanh':
        return torch.tanh(z)
    if act == 'sigmoid':
        return 1.0 / (1.0 + torch.exp(-z))
    return z


def dact_z(z, act):
    """act'(z) at the activation's INPUT (the norm kernels)."""
    one = torch.ones_like(z)
    if act == 'leaky':
        return torch.where(z > 0, one, one * 0.2)
    if act == 'relu':
        return torch.where(z > 0, one, torch.zeros_like(z))
    if act == 'tanh':
        t = torch.tanh(z)
        return 1.0 - t * t
    if act == 'sigmoid':
        t = 1.0 / (1.0 + torch.exp(-z))
        return t * (1.0 - t)
    return one


def dact_out(a, act):
    """act' through the activation's OUTPUT (pg_act_grad_from_out)."""
    one = torch.ones_like(a)
    if act == 'leaky':
        return torch.where(a > 0, one, one * 0.2)
    if act == 'relu':
        return torch.where(a > 0, one, torch.zeros_like(a))
    if act == 'tanh':
        return 1.0 - a * a
    if act == 'sigmoid':
        return a * (1.0 - a)
    return one


# ---- float64 references ------------------------------------------------------------------------------------------------------------

def norm_ref(y, g1, g2, act, p, seed, eps=EPS):
    """pg_instnorm_act_fwd / _bwd in float64: out = keep * ks * act((y - mean) * rstd) with the biased variance, dy from
    dz = (g1 + g2) * keep * ks * act'(z):  dy = (dz - mean(dz) - (y - mean) * kk) * rstd,  kk = mean(dz (y - mean)) * rstd^2.
    g1 None: forward only.  Returns a dict of everything the tolerances need."""
    ks = keep_scale(p)
    keep = mask_t(seed, y.shape, p)
    mean = y.mean(1, keepdim=True)
    xm = y - mean
    var = (xm * xm).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = xm * rstd
    r = dict(mean=mean, var=var, rstd=rstd, z=z, keep=keep, ks=ks, out=act_f(z, act) * keep * ks, y=y)
    if g1 is not None:
        g = g1 + g2 if g2 is not None else g1
        dz = g * keep * ks * dact_z(z, act)
        gm = dz.mean(1, keepdim=True)
        kk = (dz * xm).mean(1, keepdim=True) * rstd * rstd
        r.update(dz=dz, gm=gm, kk=kk, dy=(dz - gm - xm * kk) * rstd)
    return r


def act_ref(y, act, p, seed):
    """pg_act_fwd: out = keep * ks * act(y) on (npix, C)."""
    return act_f(y, act) * mask_t(seed, y.shape, p) * keep_scale(p)


def act_bwd_ref(g1, g2, a, act, p, seed):
    """pg_act_bwd from the stored POST-dropout output a: dy = (g1 + g2) * keep * ks * act'(a * (1 - p)).  a None: act' = 1."""
    g = g1 + g2 if g2 is not None else g1
    gg = g * mask_t(seed, g.shape, p) * keep_scale(p)
    if a is None:
        return dict(dy=gg, gg=gg, d=torch.ones_like(gg), ao=torch.zeros_like(gg))
    ao = a * (1.0 - float(np.float32(p))) if p > 0 else a
    d = dact_out(ao, act)
    return dict(dy=gg * d, gg=gg, d=d, ao=ao)


def softmax_ref(y):
    m = y.max(1, keepdim=True).values
    e = torch.exp(y - m)
    return e / e.sum(1, keepdim=True)


def softmax_bwd_ref(g1, g2, o):
    g = g1 + g2 if g2 is not None else g1
    return o * (g - (g * o).sum(1, keepdim=True))


# ---- plain fp32 evaluation (and its mutations) ---------------------------------------------------------------------------------------

NORM_MUTATIONS = ('mask_off_by_one', 'mask_no_sample', 'mask_bwd_transposed', 'no_keep_scale', 'g2_dropped', 'stats_first_chunk',
                  'unbiased_var', 'last_unit_neighbour_stats', 'last_pixel_nan')
ACT_MUTATIONS = ('mask_off_by_one', 'no_keep_scale', 'g2_dropped', 'last_pixel_nan', 'grad_from_scaled_out')
SOFTMAX_MUTATIONS = ('no_max_sub', 'g2_dropped', 'last_pixel_nan')


def _psum(x, reverse):
    """Sum over the pixel dim in float64; reverse: strictly sequential from the last pixel to the first."""
    x = x.double()
    if reverse:
        return torch.flip(x, (1,)).cumsum(1)[:, -1:, :]
    return x.sum(1, keepdim=True)


def _mut_mask(mut, seed, shape, p, bwd=False):
    N, HW, C = shape
    if p == 0:
        return torch.ones(shape, dtype=F32)
    if mut == 'mask_off_by_one':
        return mask_t(seed, shape, p, start=1).float()
    if mut == 'mask_no_sample':
        return mask_t(seed, (1, HW, C), p).float().expand(N, HW, C).contiguous()
    if mut == 'mask_bwd_transposed' and bwd:
        return torch.stack([mask_t(seed, (C, HW), p, start=n * HW * C).t() for n in range(N)]).float().contiguous()
    return mask_t(seed, shape, p).float()


def plain_norm(y, g1, g2, act, p, seed, mut=None, reverse=False, eps=EPS):
    """The formulas in fp32, in the header's order: plane sums in float64 rounded to fp32, z = y*rstd + (-mean*rstd), each
    operation rounded once.  Returns out, stats (N, C, 2) and dy (None without g1) as fp32 tensors."""
    N, HW, C = y.shape
    yf = y.float()
    ks = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    if mut == 'no_keep_scale':
        ks = torch.tensor(1.0, dtype=F32)
    ys = yf[:, :(HW + 1) // 2] if mut == 'stats_first_chunk' else yf
    n = ys.shape[1]
    mean64 = _psum(ys, reverse) / n
    var64 = _psum((ys.double() - mean64) ** 2, reverse) / (n - 1 if mut == 'unbiased_var' else n)
    mean, rstd = mean64.float(), (1.0 / torch.sqrt(var64 + eps)).float()
    if mut == 'last_unit_neighbour_stats':
        mean, rstd = mean.clone(), rstd.clone()
        mean[..., -1], rstd[..., -1] = mean[..., -2], rstd[..., -2]
    z = yf * rstd + (-mean * rstd)
    out = act_f(z, act)
    if p > 0:
        out = out * ks * _mut_mask(mut, seed, y.shape, p)
    stats = torch.stack([mean.view(N, C), rstd.view(N, C)], -1)
    dy = None
    if g1 is not None:
        g = g1.float() + g2.float() if (g2 is not None and mut != 'g2_dropped') else g1.float()
        if p > 0:
            g = g * ks * _mut_mask(mut, seed, y.shape, p, bwd=True)
        dz = g * dact_z(z, act)
        xm = yf - mean
        gm = (_psum(dz, reverse) / HW).float()
        kk = (_psum(dz.double() * xm.double(), reverse) * rstd.double() * rstd.double() / HW).float()
        dy = (dz - gm - xm * kk) * rstd
    if mut == 'last_pixel_nan':
        out = out.clone()
        out[-1, -1, :] = float('nan')
        if dy is not None:
            dy = dy.clone()
            dy[-1, -1, :] = float('nan')
    return out, stats, dy


def plain_act(y, act, p, seed, mut=None):
    out = act_f(y.float(), act)
    if p > 0:
        ks = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
        m = mask_t(seed, y.shape, p, start=1 if mut == 'mask_off_by_one' else 0).float()
        out = out * m if mut == 'no_keep_scale' else out * ks * m
    if mut == 'last_pixel_nan':
        out = out.clone()
        out[-1, :] = float('nan')
    return out


def plain_act_bwd(g1, g2, a, act, p, seed, mut=None):
    g = g1.float() + g2.float() if (g2 is not None and mut != 'g2_dropped') else g1.float()
    ao = a.float() if a is not None else None
    if p > 0:
        one = torch.tensor(1.0, dtype=F32)
        ks = one / (one - torch.tensor(p, dtype=F32))
        m = mask_t(seed, g.shape, p, start=1 if mut == 'mask_off_by_one' else 0).float()
        g = g * m if mut == 'no_keep_scale' else g * ks * m
        if ao is not None and mut != 'grad_from_scaled_out':
            ao = ao * (one - torch.tensor(p, dtype=F32))
    dy = g * dact_out(ao, act) if ao is not None else g
    if mut == 'last_pixel_nan':
        dy = dy.clone()
        dy[-1, :] = float('nan')
    return dy


def plain_softmax(y, mut=None):
    yf = y.float()
    e = torch.exp(yf if mut == 'no_max_sub' else yf - yf.max(1, keepdim=True).values)
    s = torch.zeros_like(e[:, :1])
    for c in range(e.shape[1]):
        s = s + e[:, c:c + 1]
    out = e / s
    if mut == 'last_pixel_nan':
        out[-1, :] = float('nan')
    return out


def plain_softmax_bwd(g1, g2, o, mut=None):
    g = g1.float() + g2.float() if (g2 is not None and mut != 'g2_dropped') else g1.float()
    of = o.float()
    dot = torch.zeros_like(of[:, :1])
    for c in range(of.shape[1]):
        dot = dot + g[:, c:c + 1] * of[:, c:c + 1]
    dy = of * (g - dot)
    if mut == 'last_pixel_nan':
        dy[-1, :] = float('nan')
    return dy


# ---- comparator --------------------------------------------------------------------------------------------------------------------

def worst_ratio(got, ref, tol, bf=False):
    """Largest |got - ref| / tol over the elements (inf for a NaN / unwritten element or a miss at tol == 0).  bf: got was stored as
    bf16 and must lie in [rne_bf16(ref - tol), rne_bf16(ref + tol)]; the ratio is 0 where got is the rounded reference itself, 1
    where it is another value of the interval, and 1 + (distance to the interval) / tol outside."""
    got, ref = got.double(), ref.double()
    tol = tol.double().expand_as(ref)
    err = (got - ref).abs()
    safe = tol.clamp_min(1e-300)
    if bf:
        lo, hi = rne_bf16(ref - tol), rne_bf16(ref + tol)
        out = torch.maximum(lo - got, got - hi).clamp_min(0.0)
        inside = torch.where(got == rne_bf16(ref), torch.zeros_like(err), torch.ones_like(err))
        ratio = torch.where(out > 0, 1.0 + out / safe, inside)
    else:
        ratio = torch.where(err == 0, torch.zeros_like(err), err / safe)
    ratio = torch.where(torch.isfinite(got) & torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    return float(ratio.max())


def tol_norm_fwd(r):
    return 4.0 * EPS32 * (r['out'].abs() + r['ks'] * (r['y'].abs() + r['mean'].abs()) * r['rstd'])


def tol_norm_bwd(r, plain_dy):
    a_b = EPS32 * r['rstd'] * (r['dz'].abs() + r['gm'].abs() + ((r['y'] - r['mean']).abs() + r['mean'].abs()) * r['kk'].abs()
                               + r['dy'].abs() / r['rstd'])
    e = (plain_dy.double() - r['dy']).abs().amax(1, keepdim=True)
    return 8.0 * (a_b + e)


def stats_ratio(stats, r):
    """(worst mean ratio, worst rstd ratio) of fp32 stats (N, C, 2) against the float64 statistics."""
    N, HW, C = r['y'].shape
    mean, var, rstd = r['mean'].view(N, C), r['var'].view(N, C), r['rstd'].view(N, C)
    rm = worst_ratio(stats[..., 0], mean, EPS32 * mean.abs())
    rr = worst_ratio(stats[..., 1], rstd, rstd * (2 * EPS32 + 2.0 ** -48 * (1 + mean * mean / (var + EPS))))
    return rm, rr


def tol_act_fwd(ref):
    return 4.0 * EPS32 * ref.abs() + 1e-37


def tol_act_bwd(r, act, p):
    s = r['ao'] ** 2 if act == 'tanh' else r['ao'].abs() if act == 'sigmoid' else torch.zeros_like(r['ao'])
    return 8.0 * EPS32 * r['gg'].abs() * (r['d'].abs() + s) + 1e-37 * r['gg'].abs()


def tol_softmax_fwd(y, ref):
    return EPS32 * (4.0 + (y - y.max(1, keepdim=True).values).abs()) * ref + 1e-37


def tol_softmax_bwd(g1, g2, o):
    g = g1 + g2 if g2 is not None else g1
    w = g.abs() + (g * o).abs().sum(1, keepdim=True)
    return 8.0 * EPS32 * o * w + 1e-37 * w


# ---- launch plan, mirrored from norm_act.hip (host side: pick_group, chunk_plan, in_apply_grid, the VEC choice) ----------------------

def pick_group(N, units):
    G = 1
    while G < 32 and G * 2 <= units and N * ((units + G * 2 - 1) // (G * 2)) >= 512:
        G *= 2
    return G


def chunk_plan(N, HW, C, vec):
    units = C // vec
    G = 1
    while G < 64 and G * 2 <= units:
        G *= 2
    groups = (units + G - 1) // G
    nchunk = 1
    if HW >= 512:
        PL = 256 // G
        want = min((1024 + N * groups - 1) // (N * groups), HW // (PL * 2), 1024)
        nchunk = max(want, 1)
    ppc = (HW + nchunk - 1) // nchunk
    nchunk = (HW + ppc - 1) // ppc
    rnd = lambda b: (b + 255) & ~255
    return dict(G=G, groups=groups, nchunk=nchunk, ppc=ppc, part_bytes=rnd(N * nchunk * C * 16), coef_bytes=rnd(N * C * 8))


def workspace_bytes(N, HW, C):
    vs = (4, 1, 8) if C % 8 == 0 else (4, 1) if C >= 4 else (1,)
    return max(sum(chunk_plan(N, HW, C, v)[k] for k in ('part_bytes', 'coef_bytes')) for v in vs)


# Layouts (ld - C, off) per storage type: 'al' 16-byte aligned with ld % 8 == C % 8 for bf16; 'ld4' bf16 at 8-byte alignment with
# ld % 8 == 4 (C % 8 == 0): VEC 4 on bf16 tensors; 'mis' off = 1 and ld = C + 3: the scalar kernels.
LAYOUT = {'al': {False: (4, 4), True: (8, 8)}, 'ld4': {False: (4, 4), True: (4, 4)}, 'mis': {False: (3, 1), True: (3, 1)}}
# storage mix -> bf16 flags of (y, out, g1/g2, dy)
MIX = {'fp32': (False, False, False, False), 'bf16': (True, True, True, True), 'y32_out16': (False, True, False, False),
       'g16_y32_dy32': (False, False, True, False)}


def vec_of(C, layout, bfs):
    """VEC of a call whose tensors have the bf16 flags `bfs`, all in `layout` (views start 256-byte aligned)."""
    ok4 = C % 4 == 0
    ok8 = C % 8 == 0 and all(bfs)
    for bf in bfs:
        pad, off = LAYOUT[layout][bf]
        ld, byte = C + pad, off * (2 if bf else 4)
        ok4 = ok4 and ld % 4 == 0 and byte % (8 if bf else 16) == 0
        ok8 = ok8 and ld % 8 == 0 and byte % 16 == 0
    return 8 if (ok4 and ok8) else 4 if ok4 else 1


NormCase = namedtuple('NormCase', 'name shape layout mix ws acts ps g2s offset scale const_ch path vec large')


def norm_plan(case, bwd=False):
    """What the dispatch of pg_instnorm_act_fwd_t / _bwd_t does with the case: VEC, path ('one-wg', 'fixed', 'flat'), G, groups,
    chunks, pixels per chunk, pixels per lane and chunk (ppl), whether the last channel group overhangs."""
    N, C, H, W = case.shape
    HW = H * W
    by, bo, bg, bd = MIX[case.mix]
    vec = vec_of(C, case.layout, (bg, bg, by, bd) if bwd else (by, bo))
    cp = chunk_plan(N, HW, C, vec)
    units = C // vec
    if cp['nchunk'] > 1 and case.ws:
        path = 'fixed' if (units <= 256 and 256 % units == 0) else 'flat'
        G, groups = cp['G'], cp['groups']
        ppl = cp['ppc'] / (256 // G)
    else:
        path, G = 'one-wg', pick_group(N, units)
        groups, ppl = (units + G - 1) // G, HW / (256 // G)
    return dict(vec=vec, path=path, G=G, groups=groups, nchunk=cp['nchunk'] if path != 'one-wg' else 1, ppc=cp['ppc'], ppl=ppl,
                overhang=groups * G > units)


def _nc(name, shape, layout='al', mix='fp32', ws=True, acts=('leaky', 'tanh'), ps=(0.0, 0.2), g2s=(False, True), offset=0.5, scale=2.0,
        const_ch=None, path='one-wg', vec=4, large=False):
    return NormCase(name, shape, layout, mix, ws, acts, ps, g2s, offset, scale, const_ch, path, vec, large)


def norm_cases():
    """The InstanceNorm table of tests/test_normact_gpu.py (its docstring names the instantiation each row reaches)."""
    cs = [
        _nc('3x6x5x7', (3, 6, 5, 7), 'mis', acts=ACTS, vec=1),
        _nc('2x8x1x2', (2, 8, 1, 2)),
        _nc('2x8x4x4', (2, 8, 4, 4), ps=(0.0, 0.2, 0.5)),
        _nc('2x8x4x4-mis', (2, 8, 4, 4), 'mis', vec=1),
        _nc('16x520x3x3', (16, 520, 3, 3)),
        _nc('16x130x3x3', (16, 130, 3, 3), 'mis', vec=1),
        _nc('2x8x16x32', (2, 8, 16, 32), acts=ACTS, path='fixed'),
        _nc('2x16x16x32-bf16', (2, 16, 16, 32), mix='bf16', path='fixed', vec=8),
        _nc('2x64x23x23', (2, 64, 23, 23), path='fixed'),
        _nc('2x64x23x23-bf16', (2, 64, 23, 23), mix='bf16', path='fixed', vec=8),
        _nc('2x24x23x23', (2, 24, 23, 23), path='flat'),
        _nc('2x24x23x23-bf16', (2, 24, 23, 23), mix='bf16', path='flat', vec=8),
        _nc('2x6x23x23', (2, 6, 23, 23), 'mis', path='flat', vec=1),
        _nc('2x6x23x23-bf16', (2, 6, 23, 23), 'mis', mix='bf16', path='flat', vec=1),
        _nc('2x2x23x23', (2, 2, 23, 23), 'mis', path='fixed', vec=1),
        _nc('2x64x23x23-nows', (2, 64, 23, 23), ws=False),
    ]
    for nm, shape, path in (('2x8x4x4', (2, 8, 4, 4), 'one-wg'), ('2x8x16x32', (2, 8, 16, 32), 'fixed'), ('2x64x23x23', (2, 64, 23, 23), 'fixed'),
                            ('2x24x23x23', (2, 24, 23, 23), 'flat')):
        cs.append(_nc(nm + '-bf16ld4', shape, 'ld4', mix='bf16', path=path))
        cs.append(_nc(nm + '-y32_out16', shape, mix='y32_out16', path=path))
        cs.append(_nc(nm + '-g16_y32_dy32', shape, mix='g16_y32_dy32', path=path))
    for nm, shape, path in (('2x8x16x32', (2, 8, 16, 32), 'fixed'), ('2x24x23x23', (2, 24, 23, 23), 'flat')):
        cs.append(_nc(nm + '-off100', shape, path=path, offset=100.0, scale=1.0))
        cs.append(_nc(nm + '-off-3', shape, path=path, offset=-3.0, scale=0.01))
    big = dict(acts=('leaky',), ps=(0.2,), g2s=(True,), path='fixed', large=True)
    cs += [_nc('8x256x64x66', (8, 256, 64, 66), **big), _nc('8x256x64x66-bf16', (8, 256, 64, 66), mix='bf16', vec=8, **big),
           _nc('8x256x64x66-mis', (8, 256, 64, 66), 'mis', vec=1, **big)]
    return cs


def const_cases():
    """A channel of constant value 1.5: z is exactly 0 and rstd = 1 / sqrt(eps) (no knife-edge nudging: the case is the edge)."""
    return [_nc('2x8x4x4-const', (2, 8, 4, 4), acts=('none', 'leaky', 'tanh'), const_ch=3),
            _nc('2x8x16x32-const', (2, 8, 16, 32), acts=('none', 'leaky', 'tanh'), const_ch=3, path='fixed'),
            _nc('2x6x23x23-const', (2, 6, 23, 23), 'mis', acts=('none', 'leaky', 'tanh'), const_ch=5, path='flat', vec=1)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def _step_bf16(y, up):
    """The next bf16 value of larger (up) / smaller magnitude."""
    b = y.float().bfloat16().view(torch.int16)
    return (b + torch.where(up, 1, -1).to(torch.int16)).view(torch.bfloat16).double()


def norm_inputs(case, seed=11):
    """(y, g1, g2, nudged fraction, left on the knife edge): y = offset + scale * randn, gradients randn, values representable in
    their tensor's storage type.  Every y whose z lies within 64 eps32 (|y| + |mean|) rstd of 0 -- where the LeakyReLU / ReLU
    derivative of a correct kernel may fall either way -- is moved away from 0 by four times that (bf16 tensors: to the next
    bf16 value), repeated until none remains."""
    N, C, H, W = case.shape
    gen = torch.Generator().manual_seed(seed)
    shape = (N, H * W, C)
    by, bo, bg, bd = MIX[case.mix]
    y = case.offset + case.scale * torch.randn(shape, generator=gen, dtype=F32).double()
    g1, g2 = torch.randn(shape, generator=gen, dtype=F32).double(), torch.randn(shape, generator=gen, dtype=F32).double()
    y = to_bf(y) if by else y.float().double()
    if bg:
        g1, g2 = to_bf(g1), to_bf(g2)
    if case.const_ch is not None:
        y[..., case.const_ch] = 1.5
        return y, g1, g2, 0.0, 0
    nudged = torch.zeros(shape, dtype=torch.bool)
    left = 0
    for _ in range(20):
        mean = y.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(1, keepdim=True) + EPS)
        z = (y - mean) * rstd
        thr = 64 * EPS32 * (y.abs() + mean.abs()) * rstd
        near = z.abs() < thr
        left = int(near.sum())
        if left == 0:
            break
        nudged |= near
        s = torch.where(z >= 0, 1.0, -1.0).double()
        if by:
            moved = torch.where(y == 0, s * 2.0 ** -10, _step_bf16(y, (y >= 0) == (s > 0)))
        else:
            moved = (y + s * 4 * thr / rstd).float().double()
        y = torch.where(near, moved, y)
    return y, g1, g2, float(nudged.double().mean()), left


def dyadic_inputs(shape, seed=5):
    """y in multiples of 1/8 with |y| <= 4: every sum and sum of squares over any chunking is exact in float64."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-32, 33, shape, generator=gen).double() / 8.0


def host_partials(y, bounds):
    """The (sum, sum of squares) partials pg_instnorm_act_fwd_parts takes, float64, over the pixel chunks [bounds[i], bounds[i+1]):
    shape (N, chunks, C, 2)."""
    parts = [torch.stack([y[:, a:b].sum(1), (y[:, a:b] ** 2).sum(1)], -1) for a, b in zip(bounds[:-1], bounds[1:])]
    return torch.stack(parts, 1).contiguous()


def chunk_bounds(HW, chunks, seed=3):
    """`chunks` non-empty pixel ranges of arbitrary sizes covering [0, HW)."""
    gen = torch.Generator().manual_seed(seed + chunks)
    cuts = sorted((torch.randperm(HW - 1, generator=gen)[:chunks - 1] + 1).tolist())
    return [0] + cuts + [HW]


# activation cases: (name, C, layout, mix ('fp32' / 'bf16'), VEC)
ACT_NPIX = 2 * 6 * 5 + 1
ACT_CASES = [('C3', 3, 'mis', 'fp32', 1), ('C8-mis', 8, 'mis', 'fp32', 1), ('C12', 12, 'al', 'fp32', 4), ('C4-bf16ld4', 4, 'ld4', 'bf16', 4),
             ('C8-bf16', 8, 'al', 'bf16', 8), ('C24-bf16', 24, 'al', 'bf16', 8)]
ACT_STRIDE_NPIX = 700001            # C = 3: 2 100 003 units > 8192 * 256: the grid-stride loop runs a second trip
PLANTED = (0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0)


def act_inputs(npix, C, bf, seed=21):
    gen = torch.Generator().manual_seed(seed + C)
    y = torch.randn((npix, C), generator=gen, dtype=F32).double() * 2
    flat = y.view(-1)
    flat[:len(PLANTED)] = torch.tensor(PLANTED, dtype=F64)
    flat[-len(PLANTED):] = torch.tensor(PLANTED, dtype=F64)
    g1, g2 = torch.randn((npix, C), generator=gen, dtype=F32).double(), torch.randn((npix, C), generator=gen, dtype=F32).double()
    if bf:
        y, g1, g2 = to_bf(y), to_bf(g1), to_bf(g2)
    else:
        y = y.float().double()
    return y, g1, g2


SOFTMAX_CS = (1, 2, 4, 7, 32)
SOFTMAX_NPIX = 2 * 9 * 7 + 1


def softmax_inputs(C, seed=31):
    """Logits randn * 3 with planted pixels: +-80 alone and together, +-100 (expf overflows without the max subtraction), equal
    logits; two gradients."""
    gen = torch.Generator().manual_seed(seed + C)
    y = (torch.randn((SOFTMAX_NPIX, C), generator=gen, dtype=F32) * 3).double()
    y[3, 0] = 80.0
    y[4, C - 1] = -80.0
    y[5, 0], y[5, C - 1] = 80.0, (-80.0 if C > 1 else 80.0)
    y[6, :] = 1.25
    y[7, 0] = 100.0
    y[8, C - 1] = -100.0
    y[-1, :] = y[-1, :] + 100.0
    y = y.float().double()
    g1, g2 = torch.randn((SOFTMAX_NPIX, C), generator=gen, dtype=F32).double(), torch.randn((SOFTMAX_NPIX, C), generator=gen, dtype=F32).double()
    return y, g1, g2


# ---- one evaluation of a case, shared by the CPU and the GPU tests ------------------------------------------------------------------

def seed_of(case):
    return SEEDS[sum(case.shape) % 3]


def combos(case):
    return [(a, p, g) for a in case.acts for p in case.ps for g in case.g2s]


def norm_ratios(case, ref, plain_dy, out, stats, dy):
    """Worst ratios of a result (out / dy: (N, HW, C), stats: (N, C, 2)) against the float64 reference `ref` of the case."""
    by, bo, bg, bd = MIX[case.mix]
    r = dict(fwd=worst_ratio(out, ref['out'], tol_norm_fwd(ref), bo))
    r['mean'], r['rstd'] = stats_ratio(stats.double(), ref)
    if dy is not None:
        r['bwd'] = worst_ratio(dy, ref['dy'], tol_norm_bwd(ref, plain_dy), bd)
    return r


def stored(x, bf):
    """What a store of the fp32 value x into a tensor of the storage type leaves, as float64."""
    return x.float().bfloat16().double() if bf else x.double()
