"""References, tolerances and the case table for the affine InstanceNorm kernels (pg_instnorm_affine_act_*; pure CPU: torch + numpy).

normact_util's scheme with gamma and beta in it: affine_ref extends normact_util.norm_ref (statistics, mask and keep scale are its
own) to float64 out / dy / d(gamma) / d(beta) in the formulas of include/patchgan_hip.h; plain_affine evaluates the same formulas in
straightforward fp32 torch ops (an emulation of no particular kernel) and carries the mutations the comparator must reject.

Tolerances, per element (eps32 = 2^-23, ks = 1 / (1 - p)); E = the largest |plain fp32 - ref| of the element's (n, c) plane, E_c the
|plain fp32 - ref| of the channel's parameter gradient, both measured from the independent evaluation and never from the library;
A_b = normact_util's plain backward bound of the element (on the dy before the multiplication by gamma):
  forward   4 eps32 (|ref| + ks ((|y| + |mean|) rstd |gamma| + |beta|)): the five roundings of a = rstd gamma, mean a, beta - mean a,
            y a, y a + b are at most half an ulp each of those magnitudes; activation and keep scale add a few ulp of the result.
  dy        8 (|gamma| A_b + eps32 |dy| + E): the plain kernel's error scaled by gamma, and the rounding of that product.
  d(beta)   4 eps32 sum |dz| + eps32 |ref| + E_c: every dz carries a few ulp (keep scale, act', the product); the sums are fp64 and
            the result is rounded to fp32 once.
  d(gamma)  8 eps32 sum |dz (y - mean)| rstd + eps32 |ref| + E_c: as d(beta), with the fp32 roundings of y - mean and rstd on top.
A bf16-stored result must lie in [rne_bf16(ref - tol), rne_bf16(ref + tol)] (normact_util.worst_ratio)."""
import torch

from tests import normact_util as U

F64, F32 = U.F64, U.F32
MUTATIONS = ('no_gamma_fwd', 'no_beta', 'no_gamma_dy', 'dgamma_no_rstd', 'param_first_sample', 'dact_unshifted')


def affine_params(C, seed=17):
    """gamma ~ U(0.5, 1.5) with a negative value, an exact 0 and an exact 1 planted; beta ~ U(-0.5, 0.5), none of them 0 (fp32 values
    as float64)."""
    gen = torch.Generator().manual_seed(seed + C)
    gamma = (torch.rand(C, generator=gen, dtype=F32) + 0.5).double()
    beta = (torch.rand(C, generator=gen, dtype=F32) - 0.5).double()
    gamma[0], gamma[1], gamma[2] = -0.75, 0.0, 1.0
    beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.25), beta)
    return gamma, beta


def affine_ref(y, g1, g2, gamma, beta, act, p, seed):
    """pg_instnorm_affine_act_fwd_t / _bwd_t in float64 on top of normact_util.norm_ref's statistics, mask and keep scale:
    z = (y - mean) rstd gamma + beta, out = keep ks act(z); dz = (g1 + g2) keep ks act'(z), s1 = sum dz, s2 = sum dz (y - mean),
    dy = (dz - s1 / HW - (y - mean) s2 rstd^2 / HW) rstd gamma, d(beta) = sum_n s1, d(gamma) = sum_n s2 rstd."""
    N, HW, C = y.shape
    r = dict(U.norm_ref(y, None, None, act, p, seed))
    ga, be = gamma.view(1, 1, C), beta.view(1, 1, C)
    xm = y - r['mean']
    z = xm * r['rstd'] * ga + be
    r.update(gamma=ga, beta=be, z=z, out=U.act_f(z, act) * r['keep'] * r['ks'])
    if g1 is not None:
        g = g1 + g2 if g2 is not None else g1
        dz = g * r['keep'] * r['ks'] * U.dact_z(z, act)
        s1, s2 = dz.sum(1, keepdim=True), (dz * xm).sum(1, keepdim=True)
        gm, kk = s1 / HW, s2 * r['rstd'] * r['rstd'] / HW
        dy0 = (dz - gm - xm * kk) * r['rstd']
        r.update(dz=dz, gm=gm, kk=kk, dy0=dy0, dy=dy0 * ga, dbeta=s1.sum(0).view(C), dgamma=(s2 * r['rstd']).sum(0).view(C),
                 abs_dz=dz.abs().sum((0, 1)), abs_dzx=((dz * xm).abs() * r['rstd']).sum((0, 1)))
    return r


def plain_affine(y, g1, g2, gamma, beta, act, p, seed, mut=None):
    """The header's formulas in fp32, each operation rounded once (plane sums in float64, as the kernels form them).  Returns a dict
    of fp32 out, stats (N, C, 2), dy, dgamma, dbeta.  mut: one of MUTATIONS."""
    N, HW, C = y.shape
    yf = y.float()
    ga, be = gamma.float().view(1, 1, C), beta.float().view(1, 1, C)
    ks = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    mean64 = yf.double().sum(1, keepdim=True) / HW
    var64 = ((yf.double() - mean64) ** 2).sum(1, keepdim=True) / HW
    mean, rstd = mean64.float(), (1.0 / torch.sqrt(var64 + U.EPS)).float()
    a = rstd * (torch.ones_like(ga) if mut == 'no_gamma_fwd' else ga)
    b = -(mean * a) if mut == 'no_beta' else be - mean * a
    z = yf * a + b
    keep = U.mask_t(seed, y.shape, p).float()
    out = U.act_f(z, act)
    if p > 0:
        out = out * ks * keep
    res = dict(out=out, stats=torch.stack([mean.view(N, C), rstd.view(N, C)], -1))
    if g1 is not None:
        g = g1.float() + g2.float() if g2 is not None else g1.float()
        if p > 0:
            g = g * ks * keep
        dz = g * U.dact_z(yf * a + (-(mean * a)) if mut == 'dact_unshifted' else z, act)
        xm = yf - mean
        s1, s2 = dz.double().sum(1, keepdim=True), (dz.double() * xm.double()).sum(1, keepdim=True)
        gm, kk = (s1 / HW).float(), (s2 * rstd.double() * rstd.double() / HW).float()
        dy = (dz - gm - xm * kk) * rstd
        t2 = s2 if mut == 'dgamma_no_rstd' else s2 * rstd.double()
        ns = slice(0, 1) if mut == 'param_first_sample' else slice(None)
        res.update(dy=dy if mut == 'no_gamma_dy' else dy * ga, dbeta=s1[ns].sum(0).view(C).float(), dgamma=t2[ns].sum(0).view(C).float())
    return res


def tol_fwd(r):
    return 4.0 * U.EPS32 * (r['out'].abs() + r['ks'] * ((r['y'].abs() + r['mean'].abs()) * r['rstd'] * r['gamma'].abs() + r['beta'].abs()))


def tol_dy(r, plain_dy):
    a_b = U.EPS32 * r['rstd'] * (r['dz'].abs() + r['gm'].abs() + ((r['y'] - r['mean']).abs() + r['mean'].abs()) * r['kk'].abs()
                                 + r['dy0'].abs() / r['rstd'])
    e = (plain_dy.double() - r['dy']).abs().amax(1, keepdim=True)
    return 8.0 * (r['gamma'].abs() * a_b + U.EPS32 * r['dy'].abs() + e)


def tol_dbeta(r, plain_dbeta):
    return 4.0 * U.EPS32 * r['abs_dz'] + U.EPS32 * r['dbeta'].abs() + (plain_dbeta.double() - r['dbeta']).abs()


def tol_dgamma(r, plain_dgamma):
    return 8.0 * U.EPS32 * r['abs_dzx'] + U.EPS32 * r['dgamma'].abs() + (plain_dgamma.double() - r['dgamma']).abs()


def ratios(case, ref, plain, got):
    """Worst |got - ref| / tol per output of a result `got` (dict of out, stats, dy, dgamma, dbeta; dy and the parameter gradients may
    be absent) against the float64 reference; `plain`: the UNMUTATED plain_affine evaluation of the same inputs."""
    by, bo, bg, bd = U.MIX[case.mix]
    r = dict(fwd=U.worst_ratio(got['out'], ref['out'], tol_fwd(ref), bo))
    r['mean'], r['rstd'] = U.stats_ratio(got['stats'].double(), ref)
    if got.get('dy') is not None:
        r['dy'] = U.worst_ratio(got['dy'], ref['dy'], tol_dy(ref, plain['dy']), bd)
    if got.get('dgamma') is not None:
        r['dgamma'] = U.worst_ratio(got['dgamma'], ref['dgamma'], tol_dgamma(ref, plain['dgamma']))
        r['dbeta'] = U.worst_ratio(got['dbeta'], ref['dbeta'], tol_dbeta(ref, plain['dbeta']))
    return r


def stored_result(case, plain):
    """What the kernels' stores would leave of a plain evaluation (out and dy in their storage types)."""
    by, bo, bg, bd = U.MIX[case.mix]
    res = dict(plain)
    res['out'] = U.stored(plain['out'], bo)
    if plain.get('dy') is not None:
        res['dy'] = U.stored(plain['dy'], bd)
    return res


def cases():
    """The smallest shapes at which each path of the affine entry points can go wrong (N x C x H x W; every case: leaky and tanh,
    p in {0, 0.2}, g2 absent and present).  path / vec: what normact_util.norm_plan must say of the case.
      single workgroup (HW < 512)   3x8x2x2 (the 2x2 bottleneck, VEC 4), 2x12x15x15 (VEC 4, three channel units), 2x5x15x15 (VEC 1)
      chunked (HW = 576)            2x64x24x24 (fixed apply), 2x12x24x24 and 2x5x24x24 (flat apply), 2x64x24x24 in bf16 (VEC 8) and
                                    with fp32 in / bf16 out"""
    return [
        U._nc('3x8x2x2', (3, 8, 2, 2)),
        U._nc('2x12x15x15', (2, 12, 15, 15)),
        U._nc('2x5x15x15', (2, 5, 15, 15), 'mis', vec=1),
        U._nc('2x64x24x24', (2, 64, 24, 24), path='fixed'),
        U._nc('2x12x24x24', (2, 12, 24, 24), path='flat'),
        U._nc('2x5x24x24', (2, 5, 24, 24), 'mis', path='flat', vec=1),
        U._nc('2x64x24x24-bf16', (2, 64, 24, 24), mix='bf16', path='fixed', vec=8),
        U._nc('2x64x24x24-y32_out16', (2, 64, 24, 24), mix='y32_out16', path='fixed'),
    ]


def workspace_bytes(N, HW, C):
    """pg_instnorm_affine_workspace_bytes: the parameter-gradient table (N * C * 16 bytes rounded up to 256) + the plain workspace."""
    return ((N * C * 16 + 255) & ~255) + U.workspace_bytes(N, HW, C)


def inputs(case, seed=11):
    """normact_util.norm_inputs of the case with the knife edge of the AFFINE z moved out of the way: every y whose
    z = (y - mean) rstd gamma + beta lies within 64 eps32 ((|y| + |mean|) rstd |gamma| + |beta|) of 0 -- where the LeakyReLU derivative
    of a correct kernel may fall either way -- is moved away (bf16 tensors: to the next bf16 value), repeated until none remains.
    Returns (y, g1, g2, gamma, beta, left on the edge)."""
    N, C, H, W = case.shape
    by = U.MIX[case.mix][0]
    y, g1, g2, frac, left = U.norm_inputs(case, seed)
    gamma, beta = affine_params(C)
    ga, be = gamma.view(1, 1, C), beta.view(1, 1, C)
    for _ in range(20):
        mean = y.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(1, keepdim=True) + U.EPS)
        z = (y - mean) * rstd * ga + be
        thr = 64 * U.EPS32 * ((y.abs() + mean.abs()) * rstd * ga.abs() + be.abs())
        near = (z.abs() < thr) & (ga != 0)
        left = int(near.sum())
        if left == 0:
            break
        s = torch.where((z >= 0) == (ga > 0), 1.0, -1.0).double()          # the direction of y that takes z away from 0
        if by:
            moved = torch.where(y == 0, s * 2.0 ** -10, U._step_bf16(y, (y >= 0) == (s > 0)))
        else:
            moved = (y + s * 4 * thr / (rstd * ga.abs()).clamp_min(1e-30)).float().double()
        y = torch.where(near, moved, y)
    return y, g1, g2, gamma, beta, left
