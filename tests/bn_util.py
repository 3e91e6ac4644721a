"""References, tolerances, launch-plan mirror and case table for the BatchNorm kernels of batchnorm.hip (pure CPU: torch + numpy).

Independent of the library, in normact_util's scheme (its dropout-mask port, activations, comparator and fp32 layouts are used, not
copied): bn_ref evaluates the formulas of include/patchgan_hip.h in float64 on the stored fp32 inputs, per SEGMENT of N / nseg
consecutive samples; plain_bn does the same in straightforward fp32 torch ops (an emulation of no particular kernel: the yardstick of
badly conditioned planes, and the carrier of the mutations the comparator must reject).  Tensors are float64 (N, HW, C) holding fp32
values -- element (n, pix, c) has dropout index (n*HW + pix)*C + c -- and results are (nseg, M, C), M = (N / nseg) * HW; the
per-(segment, channel) quantities are (nseg, 1, C).

What the kernels round (read in batchnorm.hip): sums are fp64; coef = (mean, rstd) one fp32 rounding of fp64 values each,
scale = fl(w * rstd64), shift = fl(b - mean64 * (double)scale); z = fl(fl(x * scale) + shift); xhat = fl(fl(x - mean_f) * rstd_f);
dy = scale * (dz - fl(s1 / M) - xhat * fl(s2 / M)) in fp32 (FMA contraction possible); dweight / dbias one rounding of fp64 sums of
fp32 terms; bstat stays fp64.

Tolerances, per element, never a global maximum (eps32 = 2^-23, i.e. two rounding units, as in normact_util; ks = 1 / (1 - p);
c1 = s1 / M, c2 = s2 / M; S = M * 2^-53 * mean|y|, the worst case of an fp64 sum of M terms divided by M):
  K         0 where one workgroup makes two passes over the segment (the variance is a sum of squared differences), and
            2^-48 (1 + mean^2 / (var + eps)) wherever the variance is E[x^2] - mean^2 in fp64 (the chunked path, host partials, the
            split form): normact_util.stats_ratio's term.  2^-48 = 32 * 2^-53: a value passes through about 32 fp64 additions
            (pixels per lane + the lane tree + the rows per merge lane + the merge tree), each one rounding of at most the total.
  mean      eps32 |mean| + S (one rounding).  Evaluation mode: 0, the running mean is copied.
  rstd      rstd (2 eps32 + K): stats_ratio's bound.
  scale     |scale| (eps32 + K): one rounding of w * rstd64.
  shift     eps32 |shift| + |mean| tol(scale) + |scale| S: one rounding, and the float scale it is formed from.
  out       4 (eps32 (|ref| + ks ((|y| + |mean|) |scale| + |b|)) + ks K (|y| + |mean|) |scale|): inaffine_util's forward bound with
            scale for rstd * gamma (the roundings of scale, shift, x * scale and the sum are half a unit each of those magnitudes;
            the activations have slope <= 1; activation and keep scale add a few ulp of the result), and the chunked scale's K.
  D         the error one rounding unit leaves in dz = G act'(z), G = |g1 + g2| ks keep:
            D = G (eps32 (|act'| + s) + L (eps32 ((|y| + |mean|) |scale| + |b|) + K (|y| + |mean|) |scale|)).  s = a^2 (tanh), a
            (sigmoid), 0 otherwise: 1 - t^2 and t (1 - t) turn the ulps of t into an absolute error of that size (normact_util's
            act-backward term).  L = max |act''| = 4 / (3 sqrt 3) (tanh), 1 / (6 sqrt 3) (sigmoid), 0 otherwise (the inputs stay off
            the LeakyReLU / ReLU edge): z itself is off by the forward's 1.5 eps32 ((|y| + |mean|) |scale| + |b|), five roundings
            of half a unit, which the standing multipliers cover.  With s = L = 0, D = eps32 |dz|: inaffine_util's term.  On planes
            of two values (N x C x 1 x 1) nothing else bounds it: E below is then the maximum of two samples.
  dy        8 (|scale| (D + K |dz| + mean(D) + |xhat| mean(D |xhat|) + (eps32 + K) (|c1| + (|xhat| + |mean| rstd) |c2|))
            + eps32 |dy| + E): normact_util's A_b (its kk is c2 * rstd here) scaled by |scale| with D for eps32 |dz| and what D
            leaves in c1 and c2, the rounding of the product, and E = the largest |plain fp32 - ref| of the element's (segment,
            channel), measured from plain_bn and never from the library: the backward is ill-conditioned exactly where any fp32
            evaluation loses digits (mean^2 >> var).  Evaluation mode: c1 = c2 = 0 and no mean terms.
  dbias     4 sum D + eps32 |ref| + E_c   (inaffine_util's d(beta); E_c = |plain fp32 - ref| of the channel)
  dweight   8 sum (D + K |dz|) |xhat| + eps32 |ref| + E_c   (inaffine_util's d(gamma); xhat carries scale's K)
  bstat     mean: S + 2^-52 |mean|.  Unbiased variance: M / (M - 1) times (2^-47 (var + mean^2) under K's condition -- twice K's
            relative term, as rstd = (var + eps)^(-1/2) halves it -- else M 2^-52 var) + 2^-52 var.
  moments   the split form's local (sum y, sum y^2) are fp64 sums of exactly representable terms: n * 2^-53 * sum |term|.  The
            backward's (sum dz, sum dz xhat) of a segment are held as dbias / dweight are.
  running   the header's recurrence in float64 on the kernel's own bstat, the float store after each slot: eps32 |value| per element
            (the device may contract m * q + (1 - m) * r into one fp64 FMA before the float store); num_batches_tracked exactly.
No constant other than the standing 4 and 8 multiplies a bound; 2, 2^-47, 2^-48 and 2^-52 are derived above."""
from collections import namedtuple

import numpy as np
import torch

from tests import normact_util as U

F64, F32 = U.F64, U.F32
EPS32, EPS = U.EPS32, U.EPS
KTERM = 2.0 ** -48
ACT_CURV = {'tanh': 4.0 / (3.0 * 3.0 ** 0.5), 'sigmoid': 1.0 / (6.0 * 3.0 ** 0.5)}      # max |act''|
MOMENTUM = float(np.float32(0.1))
ENTRIES = ('act_fwd', 'stats', 'act_apply', 'act_bwd', 'moments_fwd', 'moments_bwd', 'bwd_apply')
MUTATIONS = ('seg2_stats_of_seg1', 'whole_batch_stats', 'biased_bstat', 'mask_no_seg_offset', 'mask_off_by_one', 'no_keep_scale',
             'g2_dropped', 'stats_first_chunk', 'ragged_last_pixel', 'last_group_not_written', 'dweight_one_segment',
             'eval_subtracts_mean', 'shift_other_segment_mean')


# ---- float64 reference -------------------------------------------------------------------------------------------------------------

def bn_ref(y, g1, g2, w, b, act, p, seed, nseg=1, train=True, rm=None, rv=None, keep=None, eps=EPS):
    """pg_batchnorm_act_fwd / _bwd in float64.  train: batch statistics per segment; else the running statistics (nseg = 1) and
    dy = scale * dz.  g1 None: forward only.  keep: a (N, HW, C) keep mask instead of the one of (seed, p) (the split form: every rank
    draws the mask of ITS element indices)."""
    N, HW, C = y.shape
    M = (N // nseg) * HW
    ys = y.reshape(nseg, M, C)
    ks = U.keep_scale(p)
    keep = (U.mask_t(seed, y.shape, p) if keep is None else keep).reshape(nseg, M, C)
    bmean = ys.mean(1, keepdim=True)
    bvar = ((ys - bmean) ** 2).mean(1, keepdim=True)
    mean, var = (bmean, bvar) if train else (rm.view(1, 1, C), rv.view(1, 1, C))
    wv, bv = w.view(1, 1, C), b.view(1, 1, C)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = wv * rstd
    shift = bv - mean * scale
    z = ys * scale + shift
    r = dict(y=ys, M=M, nseg=nseg, train=train, mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, b=bv, z=z, keep=keep, ks=ks,
             out=U.act_f(z, act) * keep * ks, absy=ys.abs().mean(1, keepdim=True),
             moments=torch.stack([ys.sum(1), (ys * ys).sum(1)], -1), abs_moments=torch.stack([ys.abs().sum(1), (ys * ys).sum(1)], -1))
    if train:
        r['bstat'] = torch.stack([bmean.view(nseg, C), bvar.view(nseg, C) * M / max(M - 1, 1)], -1)
    if g1 is not None:
        g = g1 + g2 if g2 is not None else g1
        gk = g.reshape(nseg, M, C) * keep * ks
        da = U.dact_z(z, act)
        dz = gk * da
        xhat = (ys - mean) * rstd
        a = U.act_f(z, act)
        r.update(gk=gk.abs(), da=da.abs(), sq=a * a if act == 'tanh' else a.abs() if act == 'sigmoid' else torch.zeros_like(a),
                 lip=ACT_CURV.get(act, 0.0))
        s1, s2 = dz.sum(1, keepdim=True), (dz * xhat).sum(1, keepdim=True)
        c1, c2 = (s1 / M, s2 / M) if train else (torch.zeros_like(s1), torch.zeros_like(s2))
        r.update(dz=dz, xhat=xhat, s1=s1, s2=s2, c1=c1, c2=c2, dy=scale * (dz - c1 - xhat * c2), dweight=s2.sum(0).view(C),
                 dbias=s1.sum(0).view(C), abs_dz=dz.abs().sum(1, keepdim=True), abs_dzx=(dz * xhat).abs().sum(1, keepdim=True))
    return r


def running_ref(bstat, rm0, rv0, momentum=MOMENTUM):
    """The header's recurrence on bstat (nslots, C, 2) float64: running = (1 - m) * running + m * batch in double, stored as float
    after every slot.  Returns float64 (running_mean, running_var) holding fp32 values."""
    rm, rv = rm0.double(), rv0.double()
    for s in range(bstat.shape[0]):
        rm = (momentum * bstat[s, :, 0] + (1.0 - momentum) * rm).float().double()
        rv = (momentum * bstat[s, :, 1] + (1.0 - momentum) * rv).float().double()
    return rm, rv


# ---- plain fp32 evaluation (and its mutations) ---------------------------------------------------------------------------------------

def plain_bn(y, g1, g2, w, b, act, p, seed, nseg=1, train=True, rm=None, rv=None, mut=None, reverse=False, keep=None, eps=EPS):
    """The header's formulas in fp32, each operation rounded once; the statistics are two-pass float64 sums (in either order) rounded
    to fp32.  Returns a dict of fp32 mean / rstd / scale / shift (nseg, 1, C), out / dy (nseg, M, C), dweight / dbias (C), float64
    bstat (nseg, C, 2) and the float64 segment sums s1 / s2."""
    N, HW, C = y.shape
    Ns = N // nseg
    M = Ns * HW
    yf = y.float().reshape(nseg, M, C)
    one = torch.tensor(1.0, dtype=F32)
    ks = one if mut == 'no_keep_scale' else one / (one - torch.tensor(p, dtype=F32))
    if train:
        ystat, n = yf, M
        if mut == 'stats_first_chunk':
            ystat = yf.view(nseg, Ns, HW, C)[:, :, :(HW + 1) // 2].reshape(nseg, -1, C)
            n = ystat.shape[1]
        elif mut == 'ragged_last_pixel':                 # the pixel is missing from the sums, not from the count
            ystat = yf.view(nseg, Ns, HW, C)[:, :, :HW - 1].reshape(nseg, -1, C)
        elif mut == 'whole_batch_stats':
            ystat, n = yf.reshape(1, nseg * M, C), nseg * M
        mean64 = U._psum(ystat, reverse) / n
        var64 = U._psum((ystat.double() - mean64) ** 2, reverse) / n
        if mut == 'whole_batch_stats':
            mean64, var64 = mean64.expand(nseg, 1, C), var64.expand(nseg, 1, C)
        if mut == 'seg2_stats_of_seg1' and nseg == 2:
            mean64, var64 = mean64[:1].expand(2, 1, C), var64[:1].expand(2, 1, C)
        bstat = torch.stack([mean64.reshape(nseg, C), var64.reshape(nseg, C) * (1.0 if mut == 'biased_bstat' else n / max(n - 1, 1))], -1)
    else:
        mean64, var64, bstat = rm.float().double().view(1, 1, C), rv.float().double().view(1, 1, C), None
    rstd64 = 1.0 / torch.sqrt(var64 + eps)
    mean, rstd = mean64.float(), rstd64.float()
    scale = (w.view(1, 1, C) * rstd64).float()
    smean = mean64.flip(0) if mut == 'shift_other_segment_mean' else mean64
    shift = (b.view(1, 1, C) - smean * scale.double()).float()
    z = yf * scale + shift

    def mask():
        if keep is not None:
            return keep.float().reshape(nseg, M, C)
        if p == 0:
            return torch.ones((nseg, M, C), dtype=F32)
        if mut == 'mask_off_by_one':
            return U.mask_t(seed, (nseg, M, C), p, start=1).float()
        if mut == 'mask_no_seg_offset':
            return U.mask_t(seed, (1, M, C), p).float().expand(nseg, M, C).contiguous()
        return U.mask_t(seed, (nseg, M, C), p).float()
    km = mask()
    out = U.act_f(z, act)
    if p > 0:
        out = out * ks * km
    res = dict(mean=mean, rstd=rstd, scale=scale, shift=shift, bstat=bstat, out=out)
    if g1 is not None:
        g = g1.float() + g2.float() if (g2 is not None and mut != 'g2_dropped') else g1.float()
        g = g.reshape(nseg, M, C)
        if p > 0:
            g = g * ks * km
        dz = g * U.dact_z(z, act)
        xhat = (yf - mean) * rstd
        s1, s2 = U._psum(dz, reverse), U._psum(dz.double() * xhat.double(), reverse)
        if train or mut == 'eval_subtracts_mean':
            c1, c2 = (s1 / M).float(), (s2 / M).float()
        else:
            c1, c2 = torch.zeros_like(scale), torch.zeros_like(scale)
        ss = slice(0, 1) if mut == 'dweight_one_segment' else slice(None)
        res.update(dy=scale * (dz - c1 - xhat * c2), s1=s1, s2=s2, dweight=s2[ss].sum(0).view(C).float(), dbias=s1[ss].sum(0).view(C).float())
    if mut == 'last_group_not_written':
        for k in ('mean', 'rstd', 'scale', 'shift', 'out', 'dy', 'dweight', 'dbias'):
            if res.get(k) is not None:
                res[k] = res[k].clone()
                res[k][..., -1] = float('nan')
    return res


# ---- tolerances and the comparator ---------------------------------------------------------------------------------------------------

def kterm(r, chunked):
    """K of the module docstring, (nseg, 1, C)."""
    if not (chunked and r['train']):
        return torch.zeros_like(r['mean'])
    return KTERM * (1.0 + r['mean'] ** 2 / (r['var'] + EPS))


def _S(r):
    return r['M'] * 2.0 ** -53 * r['absy']


def tol_coef(r, chunked):
    """Tolerances of (mean, rstd, scale, shift), each (nseg, 1, C)."""
    K = kterm(r, chunked)
    S = _S(r) if r['train'] else torch.zeros_like(r['mean'])
    t_mean = EPS32 * r['mean'].abs() + S if r['train'] else torch.zeros_like(r['mean'])
    t_rstd = r['rstd'] * (2 * EPS32 + K)
    t_scale = r['scale'].abs() * (EPS32 + K)
    t_shift = EPS32 * r['shift'].abs() + r['mean'].abs() * t_scale + r['scale'].abs() * S
    return dict(mean=t_mean, rstd=t_rstd, scale=t_scale, shift=t_shift)


def tol_out(r, chunked):
    K = kterm(r, chunked)
    span = (r['y'].abs() + r['mean'].abs()) * r['scale'].abs()
    return 4.0 * (EPS32 * (r['out'].abs() + r['ks'] * (span + r['b'].abs())) + r['ks'] * K * span)


def dz_err(r, chunked):
    """D of the module docstring, (nseg, M, C): what one rounding unit does to dz."""
    span = (r['y'].abs() + r['mean'].abs()) * r['scale'].abs()
    return r['gk'] * (EPS32 * (r['da'] + r['sq']) + r['lip'] * (EPS32 * (span + r['b'].abs()) + kterm(r, chunked) * span))


def tol_dy(r, plain_dy, chunked):
    K, M = kterm(r, chunked), r['M']
    D, xh = dz_err(r, chunked), r['xhat'].abs()
    a_b = r['scale'].abs() * (D + K * r['dz'].abs() + (EPS32 + K) * (r['c1'].abs() + (xh + r['mean'].abs() * r['rstd']) * r['c2'].abs()))
    if r['train']:
        a_b = a_b + r['scale'].abs() * (D.sum(1, keepdim=True) / M + xh * (D * xh).sum(1, keepdim=True) / M)
    e = (plain_dy.double() - r['dy']).abs().amax(1, keepdim=True)
    return 8.0 * (a_b + EPS32 * r['dy'].abs() + e)


def tol_s1(r, plain_s1, chunked):
    """Tolerance of a segment's sum dz, (nseg, 1, C): dbias's formula before the sum over the segments."""
    return 4.0 * dz_err(r, chunked).sum(1, keepdim=True) + EPS32 * r['s1'].abs() + (plain_s1.double() - r['s1']).abs()


def tol_s2(r, plain_s2, chunked):
    d = (dz_err(r, chunked) + kterm(r, chunked) * r['dz'].abs()) * r['xhat'].abs()
    return 8.0 * d.sum(1, keepdim=True) + EPS32 * r['s2'].abs() + (plain_s2.double() - r['s2']).abs()


def tol_dbias(r, plain_dbias, chunked):
    return 4.0 * dz_err(r, chunked).sum((0, 1)) + EPS32 * r['dbias'].abs() + (plain_dbias.double() - r['dbias']).abs()


def tol_dweight(r, plain_dweight, chunked):
    d = (dz_err(r, chunked) + kterm(r, chunked) * r['dz'].abs()) * r['xhat'].abs()
    return 8.0 * d.sum((0, 1)) + EPS32 * r['dweight'].abs() + (plain_dweight.double() - r['dweight']).abs()


def tol_bstat(r, chunked):
    """(nseg, C, 2): batch mean and unbiased variance in fp64."""
    M, nseg = r['M'], r['nseg']
    mean, var = r['mean'].view(nseg, -1), r['var'].view(nseg, -1)
    t_mean = _S(r).view(nseg, -1) + 2.0 ** -52 * mean.abs()
    body = 2.0 ** -47 * (var + mean * mean) if chunked else M * 2.0 ** -52 * var
    return torch.stack([t_mean, body * M / max(M - 1, 1) + 2.0 ** -52 * var], -1)


def tol_moments(r, n):
    """Local forward moments (nseg, C, 2): n fp64 additions of exactly representable terms."""
    return n * 2.0 ** -53 * r['abs_moments']


def ratios(ref, plain, got, chunked):
    """Worst |got - ref| / tol per quantity present in `got` (dict: mean, rstd, scale, shift (nseg, 1, C) or coef (nseg, C, 4); bstat;
    out; dy; dweight; dbias) against the float64 reference; `plain`: the UNMUTATED plain_bn evaluation of the same inputs."""
    got = dict(got)
    if got.get('coef') is not None:
        c = got['coef'].double().reshape(ref['nseg'], 1, -1, 4)
        for i, k in enumerate(('mean', 'rstd', 'scale', 'shift')):
            got[k] = c[..., i]
    out = {}
    tc = tol_coef(ref, chunked)
    for k in ('mean', 'rstd', 'scale', 'shift'):
        if got.get(k) is not None:
            out[k] = U.worst_ratio(got[k], ref[k], tc[k])
    if got.get('bstat') is not None:
        tb = tol_bstat(ref, chunked)
        out['bmean'] = U.worst_ratio(got['bstat'][..., 0], ref['bstat'][..., 0], tb[..., 0])
        out['bvar'] = U.worst_ratio(got['bstat'][..., 1], ref['bstat'][..., 1], tb[..., 1])
    if got.get('out') is not None:
        out['out'] = U.worst_ratio(got['out'].reshape(ref['out'].shape), ref['out'], tol_out(ref, chunked))
    if got.get('dy') is not None:
        out['dy'] = U.worst_ratio(got['dy'].reshape(ref['dy'].shape), ref['dy'], tol_dy(ref, plain['dy'], chunked))
    if got.get('dweight') is not None:
        out['dweight'] = U.worst_ratio(got['dweight'], ref['dweight'], tol_dweight(ref, plain['dweight'], chunked))
        out['dbias'] = U.worst_ratio(got['dbias'], ref['dbias'], tol_dbias(ref, plain['dbias'], chunked))
    return out


def running_ratio(got_rm, got_rv, want_rm, want_rv):
    return max(U.worst_ratio(got_rm, want_rm, EPS32 * want_rm.abs()), U.worst_ratio(got_rv, want_rv, EPS32 * want_rv.abs()))


# ---- launch plan, mirrored from batchnorm.hip (host side: bn_plan, bn_small_group, bn_apply_grid, the vector / scalar decision) --------

def bn_plan(N, HW, C, vecw):
    """bn_plan is norm_act.hip's chunk_plan with its defaults (batchnorm.hip says so): normact_util's mirror of it."""
    return U.chunk_plan(N, HW, C, vecw)


def bn_small_group(units):
    G = 1
    while G < 32 and G * 2 <= units and (units + G * 2 - 1) // (G * 2) >= 64:
        G *= 2
    return G


def bn_apply_grid(N, HW, units):
    per_sample = (HW * units + 255) // 256
    return max(min((4096 + N - 1) // N, (per_sample + 3) // 4), 1)


def bad_geom(N, HW, C, nseg, minm=2):
    return N <= 0 or HW <= 0 or C <= 0 or nseg < 1 or nseg > 2 or N % nseg != 0 or N > 65535 or (N // nseg) * HW < minm


def workspace_bytes(N, HW, C, nseg):
    """pg_batchnorm_workspace_bytes: the larger partial-sum table of the vector (C >= 4) and the scalar plan + the backward's
    coefficients, each rounded up to 256 bytes; 0 for a geometry no entry point takes."""
    if bad_geom(N, HW, C, nseg, 1):
        return 0
    a = bn_plan(N, HW, C, 4)['part_bytes'] if C >= 4 else 0
    return max(a, bn_plan(N, HW, C, 1)['part_bytes']) + ((nseg * C * 8 + 255) & ~255)


def vec_of(C, layout):
    """Every tensor of a case has the case's layout, so every entry point decides alike: VEC 4 iff C % 4 == 0, ld % 4 == 0 and the
    bases are 16-byte aligned."""
    pad, off = U.LAYOUT[layout][False]
    return 4 if (C % 4 == 0 and (C + pad) % 4 == 0 and (off * 4) % 16 == 0) else 1


def bn_path(case, entry, N=None):
    """What the entry point does with the case's views (N: a local sample count, the split form's ranks).  path: 'one-wg' (the
    one-kernel forms), 'chunked-fixed' / 'chunked-flat' (k_bn_partial + merge, named by the form k_bn_apply takes for the channel
    units; the apply-only entry points are always one of these two, pg_batchnorm_stats always runs k_bn_partial)."""
    Nn, C, H, W = case.shape
    N = Nn if N is None else N
    HW = H * W
    vec = vec_of(C, case.layout)
    units = C // vec
    cp = bn_plan(N, HW, C, vec)
    fixed = units <= 256 and 256 % units == 0
    form = 'chunked-fixed' if fixed else 'chunked-flat'
    chunked = cp['nchunk'] > 1
    r = dict(vec=vec, units=units, kernels=[])
    partial = apply_ = False
    if entry in ('act_fwd', 'act_bwd'):
        partial = apply_ = chunked
    elif entry == 'stats':
        partial = True
    elif entry in ('moments_fwd', 'moments_bwd'):
        partial = chunked
    elif entry in ('act_apply', 'bwd_apply'):
        apply_ = True
    else:
        raise ValueError(entry)
    if not (partial or apply_):
        G = bn_small_group(units)
        groups = (units + G - 1) // G
        r.update(path='one-wg', G=G, groups=groups, nchunk=1, ppc=HW, ragged=False, overhang=groups * G > units, unrolled_partial=False,
                 unrolled_apply=False)
        return r
    G, groups, nchunk, ppc = cp['G'], cp['groups'], cp['nchunk'], cp['ppc']
    step = bn_apply_grid(N, HW, units) * (256 // units) if fixed else 0
    r.update(path=form, G=G, groups=groups, nchunk=nchunk, ppc=ppc, ragged=partial and nchunk * ppc != HW,
             overhang=partial and groups * G > units, unrolled_partial=partial and ppc > 3 * (256 // G),
             unrolled_apply=apply_ and fixed and 3 * step < HW,
             depth=-(-ppc // (256 // G)) + (256 // G).bit_length() + -(-(N * nchunk) // 16) + 4)
    return r


# ---- case table ----------------------------------------------------------------------------------------------------------------------

BnCase = namedtuple('BnCase', 'name shape layout nsegs acts ps g2s offset scale const_ch const_val path vec large flags')
LT = ('leaky', 'tanh')


def _bc(name, shape, layout='al', nsegs=(1, 2), acts=LT, ps=(0.0, 0.2), g2s=(False, True), offset=0.5, scale=2.0, const_ch=None,
        const_val=0.0, path='one-wg', vec=4, large=False, flags=()):
    return BnCase(name, shape, layout, nsegs, acts, ps, g2s, offset, scale, const_ch, const_val, path, vec, large, flags)


def cases():
    """N x C x H x W rows; path / vec / flags: what bn_path must say of pg_batchnorm_act_fwd and _bwd on the row (flags: 'overhang' --
    the last channel group has lanes without a channel; 'ragged' -- a shorter last pixel chunk; 'unrolled' -- the four-fold loop of
    k_bn_partial runs, and that of the fixed k_bn_apply, which smaller fixed rows reach too).  16x516x3x3 and 16x129x3x3 stand where InstanceNorm's table has 520 and 130
    channels: bn_small_group keeps 64 workgroups whatever N is, so it is 129 channel units that leave an overhanging group (G = 2)."""
    cs = [
        _bc('3x6x5x7-mis', (3, 6, 5, 7), 'mis', nsegs=(1,), acts=U.ACTS, vec=1),
        _bc('2x8x4x4', (2, 8, 4, 4)),
        _bc('2x8x4x4-mis', (2, 8, 4, 4), 'mis', vec=1),
        _bc('2x512x1x1', (2, 512, 1, 1), nsegs=(1,)),
        _bc('4x512x1x1', (4, 512, 1, 1), nsegs=(2,)),
        _bc('16x516x3x3', (16, 516, 3, 3), flags=('overhang',)),
        _bc('16x129x3x3-mis', (16, 129, 3, 3), 'mis', vec=1, flags=('overhang',)),
        _bc('2x4x16x32', (2, 4, 16, 32)),
        _bc('2x64x24x24', (2, 64, 24, 24), acts=U.ACTS, path='chunked-fixed'),
        _bc('2x64x23x25', (2, 64, 23, 25), path='chunked-fixed', flags=('ragged',)),
        _bc('2x4x32x33', (2, 4, 32, 33), path='chunked-fixed'),
        _bc('2x4x64x65-mis', (2, 4, 64, 65), 'mis', path='chunked-fixed', vec=1),
        _bc('2x1x40x41', (2, 1, 40, 41), path='chunked-fixed', vec=1, flags=('ragged',)),
        _bc('2x12x23x25', (2, 12, 23, 25), acts=U.ACTS, path='chunked-flat', flags=('overhang', 'ragged')),
        _bc('2x12x23x25-mis', (2, 12, 23, 25), 'mis', path='chunked-flat', vec=1, flags=('overhang', 'ragged')),
        _bc('2x6x23x25', (2, 6, 23, 25), path='chunked-flat', vec=1, flags=('overhang', 'ragged')),
        _bc('2x260x23x25-mis', (2, 260, 23, 25), 'mis', path='chunked-flat', vec=1, flags=('overhang', 'ragged')),
    ]
    for nm, shape, path, flags in (('2x64x23x25', (2, 64, 23, 25), 'chunked-fixed', ('ragged',)),
                                   ('2x12x23x25', (2, 12, 23, 25), 'chunked-flat', ('overhang', 'ragged'))):
        cs.append(_bc(nm + '-off100', shape, path=path, flags=flags, offset=100.0, scale=1.0))
        cs.append(_bc(nm + '-off-3', shape, path=path, flags=flags, offset=-3.0, scale=0.01))
        # a constant channel: 0 (z == shift exactly) on the fixed row, 1.5 (E[x^2] - mean^2 == 0 exactly) on the flat one
        cs.append(_bc(nm + '-const', shape, path=path, flags=flags, acts=('none', 'leaky', 'tanh'), const_ch=3,
                      const_val=0.0 if path == 'chunked-fixed' else 1.5))
    cs.append(_bc('8x512x32x33', (8, 512, 32, 33), acts=('leaky',), ps=(0.2,), g2s=(True,), path='chunked-fixed', large=True,
                  flags=('ragged', 'unrolled')))
    return cs


def modes(case):
    """(train, nseg) of every run of a row: training mode with the row's segment counts, evaluation mode with one."""
    return [(True, s) for s in case.nsegs] + [(False, 1)]


def combos(case):
    return [(a, p, g) for a in case.acts for p in case.ps for g in case.g2s]


def seed_of(case):
    return U.SEEDS[sum(case.shape) % 3]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def bn_params(C, seed=17):
    """weight ~ U[0.5, 1.5) with a negative value and an exact 0 planted where C >= 4; bias ~ U(-0.5, 0.5), |bias| >= 0.05 (fp32
    values as float64)."""
    gen = torch.Generator().manual_seed(seed + C)
    w = (torch.rand(C, generator=gen, dtype=F32) + 0.5).double()
    b = (torch.rand(C, generator=gen, dtype=F32) - 0.5).double()
    if C >= 4:
        w[0], w[1] = -0.75, 0.0
    b = torch.where(b.abs() < 0.05, torch.full_like(b, 0.25), b)
    return w, b


def _z_of(y, w, b, nseg, train, rm, rv):
    N, HW, C = y.shape
    ys = y.reshape(nseg, -1, C)
    if train:
        mean = ys.mean(1, keepdim=True)
        var = ((ys - mean) ** 2).mean(1, keepdim=True)
    else:
        mean, var = rm.view(1, 1, C), rv.view(1, 1, C)
    scale = w.view(1, 1, C) / torch.sqrt(var + EPS)
    z = ys * scale + (b.view(1, 1, C) - mean * scale)
    thr = 64 * EPS32 * ((ys.abs() + mean.abs()) * scale.abs() + b.view(1, 1, C).abs())
    return z.reshape(y.shape), thr.reshape(y.shape), scale.expand_as(ys).reshape(y.shape)


def inputs(case, seed=11):
    """dict of y, g1, g2 (N, HW, C), w, b, rm, rv (C) as float64 holding fp32 values, the nudged fraction `frac` and the number
    `left` on the knife edge.  y = offset_c + scale_c * randn with a per-channel offset and scale around the case's; running
    statistics near the batch's.  Every y whose z = y * scale + shift lies within 64 eps32 ((|y| + |mean|) |scale| + |b|) of 0 in ANY
    mode of the row -- where the LeakyReLU / ReLU derivative of a correct kernel may fall either way -- is moved away from it by four
    times that (and two times more with every round: the modes' edges lie apart, and a fixed step could hand an element back and
    forth between two of them), repeated until none remains in any mode (channels of weight 0 and the constant channel have z = b or
    next to it).  `frac` is the largest nudged fraction of one mode: the modes' edges are different elements, a row of three modes
    moves three times as many."""
    N, C, H, W = case.shape
    gen = torch.Generator().manual_seed(seed)
    shape = (N, H * W, C)
    off = case.offset + 0.25 * case.scale * torch.randn(C, generator=gen, dtype=F32).double()
    sc = case.scale * (0.5 + torch.rand(C, generator=gen, dtype=F32).double())
    y = (off + sc * torch.randn(shape, generator=gen, dtype=F32).double()).float().double()
    g1, g2 = torch.randn(shape, generator=gen, dtype=F32).double(), torch.randn(shape, generator=gen, dtype=F32).double()
    rm = (off + 0.1 * sc * torch.randn(C, generator=gen, dtype=F32).double()).float().double()
    rv = (sc * sc * (0.5 + torch.rand(C, generator=gen, dtype=F32).double())).float().double()
    w, b = bn_params(C)
    live = (w != 0).view(1, 1, C).expand(shape).clone()
    if case.const_ch is not None:
        y[..., case.const_ch] = case.const_val
        live[..., case.const_ch] = False
    ms = modes(case)
    nudged = [torch.zeros(shape, dtype=torch.bool) for _ in ms]
    left = 0
    for it in range(20):
        left = 0
        for i, (train, nseg) in enumerate(ms):
            z, thr, scale = _z_of(y, w, b, nseg, train, rm, rv)
            near = (z.abs() < thr) & live
            k = int(near.sum())
            left += k
            if k:
                nudged[i] |= near
                s = torch.where((z >= 0) == (scale > 0), 1.0, -1.0).double()
                y = torch.where(near, (y + s * (4 + 2 * it) * thr / scale.abs().clamp_min(1e-30)).float().double(), y)
        if left == 0:
            break
    frac = max(float(m.double().mean()) for m in nudged)
    return dict(y=y, g1=g1, g2=g2, w=w, b=b, rm=rm, rv=rv, frac=frac, left=left)


def evaluate(case, inp, train, nseg, act, p, g2on, mut=None, reverse=False, keep=None):
    """(ref, plain) of one run of a row."""
    g2 = inp['g2'] if g2on else None
    seed = seed_of(case)
    ref = bn_ref(inp['y'], inp['g1'], g2, inp['w'], inp['b'], act, p, seed, nseg, train, inp['rm'], inp['rv'], keep=keep)
    plain = plain_bn(inp['y'], inp['g1'], g2, inp['w'], inp['b'], act, p, seed, nseg, train, inp['rm'], inp['rv'], mut=mut, reverse=reverse, keep=keep)
    return ref, plain
