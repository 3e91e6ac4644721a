"""References, bounds and case tables for the spectral-normalisation kernels (pg_spectral_fwd / pg_spectral_bwd; pure CPU: torch).

`power_step` / `grad_map` evaluate the formulas of include/patchgan_hip.h on torch-layout tensors (W [Cout, Cin, 4, 4], Wm =
W.reshape(Cout, Cin*16), u [Cout], v [Cin*16]) in float64 -- the reference -- or, with store=torch.float32, as an emulation of the
kernels' arithmetic: fp64 sums, every stored result (v, u, sigma, w_hat, dW) rounded to fp32 once and USED rounded by the stages after
it.  The emulation carries the mutations the comparator must reject (MUTATIONS).

Bounds (eps32 = 2^-23), per element, from the header's arithmetic: a stored float is ONE rounding of an fp64 expression of stored
fp32 values, so it lies within eps32/2 |ref| of the float64 evaluation of the same expression on the same stored inputs (the fp64
sums' own error, ~n 2^-53 of the sum of magnitudes, is nine orders below).  The tests allow 4 eps32 |ref| for u, v, sigma, w_hat and
4 eps32 (|dW_hat| + |c u_o v_k|) / sigma for dW -- the constants the feature's specification names; the arithmetic needs no other --
and evaluate the reference STAGE BY STAGE on what the kernel stored (`stage_ratios`): v from the given u, u from the stored v, sigma
from the stored u and v, w_hat from the stored sigma, dW from the stored w_hat, u, v, sigma.
"""
import torch

F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -23
EPS = 1e-12
MUTATIONS = ('dw_no_second_term', 'sigma_old_u', 'v_packed_order', 'no_eps', 'bias_scaled')

# (Cout, Cin): odd Cin and tail lanes; a scalar u; neither a power of two; the benchmark's largest layer (several workgroups per sum)
KERNEL_SHAPES = [(8, 5), (1, 64), (40, 24), (512, 256)]


def pack(W):
    """torch [Cout, Cin, 4, 4] -> the packed block [16 taps][Cout][Cin], flat."""
    return W.permute(2, 3, 0, 1).reshape(-1).contiguous()


def unpack(P, a, b):
    return P.reshape(4, 4, a, b).permute(2, 3, 0, 1)


def layer_inputs(a, b, seed=0):
    """fp32 W (kaiming-uniform scale, as torch's conv init), unit u, v, and an upstream gradient dW_hat, as float32 tensors."""
    gen = torch.Generator().manual_seed(1000 * a + b + seed)
    bound = 1.0 / (b * 16) ** 0.5
    W = torch.empty(a, b, 4, 4).uniform_(-bound, bound, generator=gen)
    u = torch.nn.functional.normalize(torch.randn(a, generator=gen), dim=0, eps=EPS)
    v = torch.nn.functional.normalize(torch.randn(b * 16, generator=gen), dim=0, eps=EPS)
    g = torch.randn(a, b, 4, 4, generator=gen) * 0.01
    return W, u, v, g


def _st(x, store):
    return x if store is None else x.to(store).double()


def power_step(W, u, v, iterate, store=None, mut=None):
    """One pg_spectral_fwd item: dict of v, u, sigma, w_hat (float64 tensors; with store=torch.float32 each is a float32 value).
    store=None: the float64 reference, nothing rounded."""
    a = W.shape[0]
    Wm = W.double().reshape(a, -1)
    u, v = u.double(), v.double()
    u_old = u
    if iterate:
        t = Wm.t() @ u
        nt = t.norm()
        v = _st(t / (nt if mut == 'no_eps' else nt.clamp_min(EPS)), store)
        if mut == 'v_packed_order':        # v left in the packed (tap, ci) order instead of torch's (ci, tap)
            v = v.reshape(-1, 16).t().reshape(-1).contiguous()
    s = Wm @ v
    if iterate:
        ns = s.norm()
        u = _st(s / (ns if mut == 'no_eps' else ns.clamp_min(EPS)), store)
    sigma = _st(((u_old if mut == 'sigma_old_u' else u) * s).sum(), store)
    return dict(v=v, u=u, sigma=sigma, w_hat=_st(W.double() / sigma, store))


def grad_map(g, w_hat, u, v, sigma, store=None, mut=None):
    """One pg_spectral_bwd item: dW = (dW_hat - <dW_hat, W_hat> u v^T) / sigma, torch layout, float64 (rounded once with `store`)."""
    g, w_hat = g.double(), w_hat.double()
    c = (g * w_hat).sum()
    uv = (u.double().view(-1, 1) * v.double().view(1, -1)).reshape(g.shape)
    corr = torch.zeros_like(g) if mut == 'dw_no_second_term' else c * uv
    return _st((g - corr) / sigma.double(), store), c, uv


def ratio(got, ref, tol):
    """Worst |got - ref| / tol; inf where got is not finite."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float(((got - ref).abs() / tol.double().reshape(-1).clamp_min(1e-300)).max())


def stage_ratios(W, u0, v0, got, iterate, g=None):
    """Worst error / bound per output of a result `got` (dict of v, u, sigma, w_hat and, with g, dW: what a kernel or the emulation
    stored) for fp32 inputs W, u0, v0 (and upstream gradient g): the float64 reference of each stage on the STORED values before it."""
    a = W.shape[0]
    Wm = W.double().reshape(a, -1)
    r = {}
    if iterate:
        t = Wm.t() @ u0.double()
        ref_v = t / t.norm().clamp_min(EPS)
        r['v'] = ratio(got['v'], ref_v, 4 * EPS32 * ref_v.abs())
        s = Wm @ got['v'].double()
        ref_u = s / s.norm().clamp_min(EPS)
        r['u'] = ratio(got['u'], ref_u, 4 * EPS32 * ref_u.abs())
    else:
        r['v'] = 0.0 if torch.equal(got['v'].double(), v0.double()) else float('inf')
        r['u'] = 0.0 if torch.equal(got['u'].double(), u0.double()) else float('inf')
    ref_sigma = (got['u'].double() * (Wm @ got['v'].double())).sum()
    r['sigma'] = ratio(got['sigma'], ref_sigma, 4 * EPS32 * ref_sigma.abs())
    ref_w = W.double() / got['sigma'].double()
    r['w_hat'] = ratio(got['w_hat'], ref_w, 4 * EPS32 * ref_w.abs())
    if g is not None:
        ref_dw, c, uv = grad_map(g, got['w_hat'], got['u'], got['v'], got['sigma'])
        r['dW'] = ratio(got['dW'], ref_dw, 4 * EPS32 * (g.double().abs() + (c * uv).abs()) / got['sigma'].double().abs())
    return r


def emulate(W, u0, v0, iterate, g=None, mut=None):
    """The kernels' arithmetic on one layer (fp32 stores): dict of v, u, sigma, w_hat (+ dW)."""
    got = power_step(W, u0, v0, iterate, store=F32, mut=mut)
    if g is not None:
        got['dW'] = grad_map(g, got['w_hat'], got['u'], got['v'], got['sigma'], store=F32, mut=mut)[0]
    return got


def effective_flat(flat, layers, sigmas, mut=None):
    """The effective-weight buffer of a flat parameter buffer: each normalised layer's block divided by its sigma, everything else
    copied (float32).  mut 'bias_scaled': the bias blocks divided as well."""
    eff = flat.clone()
    for l, sg in zip([l for l in layers if l.sn], sigmas):
        n = 16 * l.a * l.b
        eff[l.p_off:l.p_off + n] = (flat[l.p_off:l.p_off + n].double() / float(sg)).float()
        if mut == 'bias_scaled' and l.bias_key is not None:
            eff[l.b_off:l.b_off + l.cout] = (flat[l.b_off:l.b_off + l.cout].double() / float(sg)).float()
    return eff


def sample(t, full_max=4096):
    """tests/golden/make_golden_sn.py's `pick`: the elements of a tensor the fixtures store."""
    f = t.detach().flatten().cpu()
    if f.numel() > full_max:
        f = f[torch.arange(full_max, dtype=torch.int64) * 2654435761 % f.numel()]
    return f


def rel_dist(a, b):
    """Largest |a - b| relative to the largest |b| (float64)."""
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
