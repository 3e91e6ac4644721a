"""A plain model of the four stride-1 Winograd algorithms of patchgan_amd/csrc/conv_wino.hip -- F(2x2,4x4) / F(3x3,4x4) forward and
data gradient, F(4x4,2x2) / F(4x4,3x3) weight gradient -- and the statistic that holds the kernels to float64 element by element
(tests/test_wino1_cpu.py, tests/test_wino1_gpu.py).

These kernels are the one conv class tests/test_exact_gpu.py leaves out: their tables hold 1/3, 1/6 and 1/15, so no operand makes
their fp32 arithmetic exact.  What can be asked of them instead: the error of each output element against float64, in units of
what the element was summed from, is no larger than the error THE ALGORITHM makes in fp32 on the same operands.  The model below is
that yardstick: device-agnostic torch, the arithmetic in `dtype`, transforms as einsums, one matmul per transform point.  It is not
a bit model of the kernels (summation order and FMA contraction differ).  Run in float64 it equals the convolution (the CPU test),
which proves the tables, the window origins, the tap flip and the ragged edges of the yardstick itself.

Statistic (Stat / within): e_i = |got_i - ref_i| / S_i with ref the float64 result and S the same convolution of the absolute
values (|x| * |w| + |bias|; weight gradient: sum |dy| |x|).  A kernel result passes when max e <= 4 max e(model in fp32) and
rms e <= 2 rms e(model): 4 is the project's standing margin over the reference's own fp32-vs-float64 distance (summation order,
extreme-value scatter); the rms of ~10^6 elements barely scatters, and a lost bit of precision doubles it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import exact_util as X

MAX_FACTOR, RMS_FACTOR = 4.0, 2.0

# the transform tables of conv_wino.hip as float64 (the CPU test compares their fp32 roundings with the source)
c_BT = np.array([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], np.float64)
c_G = np.array([[1 / 2, 0, 0, 0], [-1 / 2, -1 / 2, -1 / 2, -1 / 2], [-1 / 6, 1 / 6, -1 / 6, 1 / 6], [1 / 6, 1 / 3, 2 / 3, 4 / 3], [0, 0, 0, 1]], np.float64)
c_AT24 = np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 1]], np.float64)
c_BT6 = np.array([[1, -1.5, -2, 1.5, 1, 0], [0, -1, 0.5, 2.5, 1, 0], [0, 1, -2.5, 0.5, 1, 0], [0, -2, -1, 2, 1, 0], [0, 0.5, -1, -0.5, 1, 0],
                  [0, 1, -1.5, -2, 1.5, 1]], np.float64)
c_G34 = np.array([[1, 0, 0, 0], [1 / 3, 1 / 3, 1 / 3, 1 / 3], [-1 / 3, 1 / 3, -1 / 3, 1 / 3], [-16 / 15, -8 / 15, -4 / 15, -2 / 15],
                  [1 / 15, -2 / 15, 4 / 15, -8 / 15], [0, 0, 0, 1]], np.float64)
c_AT34 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 1]], np.float64)
c_G2 = np.array([[1 / 2, 0], [-1 / 2, -1 / 2], [-1 / 6, 1 / 6], [1 / 6, 1 / 3], [0, 1]], np.float64)
c_A4T = np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 0], [0, 1, -1, 8, 1]], np.float64)
c_G43 = np.array([[1, 0, 0], [1 / 3, 1 / 3, 1 / 3], [-1 / 3, 1 / 3, -1 / 3], [-16 / 15, -8 / 15, -4 / 15], [1 / 15, -2 / 15, 4 / 15], [0, 0, 1]], np.float64)
c_A4T6 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 0], [0, 1, -1, 0.125, -8, 1]], np.float64)
TABLES = {'c_BT': c_BT, 'c_G': c_G, 'c_AT24': c_AT24, 'c_BT6': c_BT6, 'c_G34': c_G34, 'c_AT34': c_AT34, 'c_G2': c_G2, 'c_A4T': c_A4T,
          'c_G43': c_G43, 'c_A4T6': c_A4T6}
FWD_TABLES = {2: (c_BT, c_G, c_AT24), 3: (c_BT6, c_G34, c_AT34)}        # (B^T, G, A^T) by output tile edge
WGRAD_TABLES = {2: (c_BT, c_G2, c_A4T), 3: (c_BT6, c_G43, c_A4T6)}      # ... by dy tile edge


def _tables(three, dtype, device):
    """The tables as the kernels hold them (fp32 constants), carried in `dtype`; float64 keeps the exact-to-double fractions."""
    f = (lambda t: t) if dtype == torch.float64 else (lambda t: t.astype(np.float32))
    return tuple(torch.from_numpy(f(t)).to(device=device, dtype=dtype) for t in three)


def matmul_gemm(A, B):
    """M[p] = A[p] B[p]^T, A [points, rows, K], B [points, cols, K]: one matmul per transform point."""
    return A @ B.transpose(1, 2)


def chunk_gemm(A, B, kc=32, order=None, skip=()):
    """The same sums taken K chunk by K chunk in `order` (default ascending), every chunk's product added in the operands' type.
    skip: (point, chunk) pairs left out -- a damaged GEMM for the sensitivity tests."""
    nch = (A.shape[2] + kc - 1) // kc
    acc = torch.zeros(A.shape[0], A.shape[1], B.shape[1], dtype=A.dtype, device=A.device)
    for c in (range(nch) if order is None else order):
        part = A[:, :, c * kc:(c + 1) * kc] @ B[:, :, c * kc:(c + 1) * kc].transpose(1, 2)
        for p, cc in skip:
            if cc == c:
                part[p] = 0
        acc = acc + part
    return acc


def _windows(x, pad, step, TH, TW):
    """[N, C, TH, TW, step + 3, step + 3]: the windows at (step ti - pad, step tj - pad) of x, zero outside (k_wino_v)."""
    H, W = x.shape[2:]
    xp = F.pad(x, (pad, step * TW + 3 - pad - W, pad, step * TH + 3 - pad - H))
    return xp.unfold(2, step + 3, step).unfold(3, step + 3, step)


def tiles(extent, edge):
    return (extent + edge - 1) // edge


def _corr_model(x, Wc, pad, mo, dtype, gemm, damage_m=None):
    """out[n, o, y, x] = sum_{c, i, j} x[n, c, y - pad + i, x - pad + j] Wc[o, c, i, j] by F(mo x mo, 4x4)."""
    BT, G, AT = _tables(FWD_TABLES[mo], dtype, x.device)
    x, Wc = x.to(dtype), Wc.to(dtype)
    N, Ci, H, W = x.shape
    Co, NP = Wc.shape[0], mo + 3
    Ho, Wo = H + 2 * pad - 3, W + 2 * pad - 3
    TH, TW = tiles(Ho, mo), tiles(Wo, mo)
    V = torch.einsum('ai,nchwij,bj->abnhwc', BT, _windows(x, pad, mo, TH, TW), BT).reshape(NP * NP, N * TH * TW, Ci)
    U = torch.einsum('ak,ockl,bl->aboc', G, Wc, G).reshape(NP * NP, Co, Ci)
    M = (gemm or matmul_gemm)(V, U)
    if damage_m is not None:
        M = damage_m(M, V, U)
    M = M.reshape(NP, NP, N, TH, TW, Co)
    out = torch.einsum('pa,abnhwo,qb->nohpwq', AT, M, AT).reshape(N, Co, TH * mo, TW * mo)
    return out[:, :, :Ho, :Wo]


def _epilogue(out, bias, act, dtype):
    if bias is not None:
        out = out + bias.to(dtype).view(1, -1, 1, 1)
    assert act in ('none', 'leakyrelu')
    return F.leaky_relu(out, 0.2) if act == 'leakyrelu' else out


def wino1_fwd_model(x, Wt, mo, dtype, bias=None, act='none', gemm=None, damage_m=None):
    """big [N, Cb, Hb, Wb] -> small [N, Ca, Hb - 1, Wb - 1] of a stride-1 layer, Wt [Ca, Cb, 4, 4]: the pad-1 correlation."""
    return _epilogue(_corr_model(x, Wt, 1, mo, dtype, gemm, damage_m), bias, act, dtype)


def wino1_dgrad_model(dy, Wt, mo, dtype, bias=None, act='none', gemm=None, damage_m=None):
    """small [N, Ca, Hs, Ws] -> big [N, Cb, Hs + 1, Ws + 1]: the pad-2 correlation with flipped taps and swapped channel roles, on the
    same tables."""
    return _epilogue(_corr_model(dy, Wt.flip(2, 3).transpose(0, 1), 2, mo, dtype, gemm, damage_m), bias, act, dtype)


def wino1_wgrad_model(x, dy, r, dtype, gemm=None):
    """dW [Ca, Cb, 4, 4] from big x [N, Cb, Hb, Wb] and dy [N, Ca, Hb - 1, Wb - 1] by F(4x4, r x r): r x r tiles of dy (zero beyond
    the last row / column) against the (r + 3)^2 windows of x at (r ti - 1, r tj - 1); the GEMMs reduce over the tiles."""
    BT, G, AT = _tables(WGRAD_TABLES[r], dtype, x.device)
    x, dy = x.to(dtype), dy.to(dtype)
    N, Cb = x.shape[:2]
    _, Ca, Hs, Ws = dy.shape
    TH, TW, NP = tiles(Hs, r), tiles(Ws, r), r + 3
    V = torch.einsum('ai,nchwij,bj->abnhwc', BT, _windows(x, 1, r, TH, TW), BT).reshape(NP * NP, N * TH * TW, Cb)
    dyp = F.pad(dy, (0, r * TW - Ws, 0, r * TH - Hs)).reshape(N, Ca, TH, r, TW, r)
    DY = torch.einsum('au,nchuwv,bv->abnhwc', G, dyp, G).reshape(NP * NP, N * TH * TW, Ca)
    S = (gemm or matmul_gemm)(DY.transpose(1, 2), V.transpose(1, 2)).reshape(NP, NP, Ca, Cb)
    return torch.einsum('ki,ijab,lj->abkl', AT, S, AT)


# ---- operands, float64 references and the statistic -----------------------------------------------------------------------------
def normal_operands(geom, seed=0, device='cpu'):
    """i.i.d. normal operands scaled as tests/test_fuzz_gpu.py scales them (outputs of order 1 in both directions, S near-uniform)."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    g = X._gen(geom, 1000 + seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    big, small = rn(N, Cb, Hb, Wb), rn(N, Ca, Hs, Ws)
    Wt = rn(Ca, Cb, 4, 4) / math.sqrt(max(Ca, Cb) * 16)
    ops = X.Operands(geom, big, small, Wt, rn(Ca), rn(Cb))
    return on_device(ops, device)


def on_device(ops, device):
    c = lambda t: t.to(device) if t is not None else None
    return X.Operands(ops.geom, c(ops.big), c(ops.small), c(ops.Wt), c(ops.bias_a), c(ops.bias_b), ops.lsb)


def replaced(ops, **kw):
    d = dict(big=ops.big, small=ops.small, Wt=ops.Wt, bias_a=ops.bias_a, bias_b=ops.bias_b)
    d.update(kw)
    return X.Operands(ops.geom, d['big'], d['small'], d['Wt'], d['bias_a'], d['bias_b'], ops.lsb)


def _abs(ops):
    a = lambda t: t.abs() if t is not None else None
    return X.Operands(ops.geom, a(ops.big), a(ops.small), a(ops.Wt), a(ops.bias_a), a(ops.bias_b), ops.lsb)


def ref_and_scale(ops, op, act='none', bias=True):
    """(float64 reference, S) of opcode `op` on the device the operands live on (exact_util.reference64).  S: the same convolution
    of the absolute values -- |x| * |w| + |bias|; op 2: sum |dy| |x| for dW (its dbias is not returned here).  LeakyReLU is
    1-Lipschitz: the same S bounds the activated result."""
    ref, S = X.reference64(ops, op, 'none', bias), X.reference64(_abs(ops), op, 'none', bias)
    if op == 2:
        return ref[0], S[0]
    return (F.leaky_relu(ref, 0.2) if act == 'leakyrelu' else ref), S


class Stat:
    """max and rms of e_i = |got_i - ref_i| / S_i (or / one normaliser for the whole selection).  maxnorm: max |got - ref| / max |ref|,
    the one ratio the older tolerance tests look at (reported only)."""

    def __init__(self, got, ref, S, where=None, norm=None):
        assert got.shape == ref.shape, (got.shape, ref.shape)
        d = (got.double() - ref).abs()
        e = d / norm if norm is not None else d / S
        self.maxnorm = float(d.max() / ref.abs().max())
        if where is not None:
            e = e[where]
        self.n = e.numel()
        self.nan = int(e.isnan().sum())
        self.max = float(e.max()) if not self.nan else float('nan')
        self.rms = float(e.square().mean().sqrt()) if not self.nan else float('nan')
        s = S if where is None else S[where]
        self.spread = float(s.max() / s.min()) if float(s.min()) > 0 else float('inf')

    def __repr__(self):
        return f'max e {self.max:.3e} rms e {self.rms:.3e}'


def within(kernel, model):
    """The step-2 bound.  NaN on either side fails."""
    return (kernel.nan == 0 and model.nan == 0 and kernel.max <= MAX_FACTOR * model.max and kernel.rms <= RMS_FACTOR * model.rms)


def report(what, kernel, model):
    return (f'{what}: model max e {model.max:.3e} rms e {model.rms:.3e} | kernel max e {kernel.max:.3e} ({kernel.max / model.max:.2f}x) '
            f'rms e {kernel.rms:.3e} ({kernel.rms / model.rms:.2f}x) | max S / min S {kernel.spread:.2f} | max-norm ratio {kernel.maxnorm:.2e}')


# ---- isolation probes ---------------------------------------------------------------------------------------------------------------
def corner_input(x):
    """x with everything but the last sample's last two rows and last two columns zeroed."""
    out = torch.zeros_like(x)
    out[-1, :, -2:, :] = x[-1, :, -2:, :]
    out[-1, :, :, -2:] = x[-1, :, :, -2:]
    return out


def quiet_mask(N, H, W, pad, mo, device='cpu'):
    """[N, Ho, Wo] bool: output elements of the tiles whose whole input window misses what corner_input keeps -- every tile of every
    sample but the last, and in the last sample the tiles whose (mo + 3)^2 window at (mo ti - pad, mo tj - pad) ends before row H - 2 and
    before column W - 2.  Such a tile's transformed input is exactly zero, so its outputs are the bias exactly."""
    Ho, Wo = H + 2 * pad - 3, W + 2 * pad - 3
    ti, tj = torch.arange(Ho, device=device) // mo, torch.arange(Wo, device=device) // mo
    rows_ok, cols_ok = mo * ti - pad + mo + 2 < H - 2, mo * tj - pad + mo + 2 < W - 2
    q = torch.ones(N, Ho, Wo, dtype=torch.bool, device=device)
    q[-1] = rows_ok[:, None] & cols_ok[None, :]
    return q


def probe_stats(got, ref, S, bias, quiet):
    """(quiet-tile elements that are not == their bias, Stat of all the others).  The others all lie in the last sample; they are
    normalised by that sample's max S, because S_i vanishes where only transform leakage arrives."""
    q = quiet[:, None].expand_as(got)
    want = (bias.view(1, -1, 1, 1) if bias is not None else torch.zeros(1, 1, 1, 1, device=got.device)).to(got.dtype).expand_as(got)
    bad = int((~(got == want) & q).sum())
    return bad, Stat(got, ref, S, where=~q, norm=S[-1].max())


def last_tile_dy(dy, r):
    """dy with everything but the last sample's last (ragged) r x r tile zeroed."""
    Hs, Ws = dy.shape[2:]
    out = torch.zeros_like(dy)
    y0, x0 = r * (tiles(Hs, r) - 1), r * (tiles(Ws, r) - 1)
    out[-1, :, y0:, x0:] = dy[-1, :, y0:, x0:]
    return out


# ---- the planner's rules the case lists are built on (conv_wino.hip; ConvOp has no query for them) ---------------------------------
def fwd_tile_edge(sym):
    """Output tile edge of a stride-1 forward / data-gradient kernel symbol."""
    if sym.startswith(('k_wino_gemm_row', 'k_wino_gemm_dma<3')) or (sym.startswith('k_wino_gemm<') and sym.endswith(',3>')):
        return 3
    assert sym.startswith(('k_wino_gemm<', 'k_wino_gemm_dma<2')), sym
    return 2


def fwd_slices(N, Ho, Wo, Cin, Cout):
    """pg_wino_gemm_slices of the F(3x3,4x4) instance: the fewest of 1 / 2 / 4 K slices that give >= 400 workgroups.  (The slab reduce
    follows only the fully fused kernel: the row-split form never slices.)"""
    wg = tiles(N * tiles(Ho, 3) * tiles(Wo, 3), 64) * tiles(Cout, 64)
    nch = Cin // 64
    if wg >= 400:
        return 1
    if nch % 2 == 0 and (wg * 2 >= 400 or nch % 4 != 0):
        return 2
    return 4 if nch % 4 == 0 else 1


def wgrad_r(N, Hs, Ws):
    """pg_wino_wgrad_r: dy tile edge 3 where that leaves >= 1024 tiles."""
    return 3 if N * tiles(Hs, 3) * tiles(Ws, 3) >= 1024 else 2
