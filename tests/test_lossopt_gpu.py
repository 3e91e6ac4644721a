"""The loss kernels of loss.hip and the Adam / bf16-padding kernels of optim_layout.hip against float64, element by element.

Calls go through the C ABI (patchgan_amd._lib) on guarded views (tests/guard_util.py: what a kernel fails to write, or reads beside
its slice, is an all-ones NaN and fails the comparison).  References, tolerances, inputs and case tables live in
tests/lossopt_util.py; tests/test_lossopt_cpu.py shows without a GPU that they accept a plain fp32 evaluation and reject the seeded
mutations.  Every test prints its worst |got - ref| / tol, and asserts the kernel path by the library's own answers
(pg_loss_reduce_doubles, the return value of pg_loss_reduce_parts).

  test                              kernels
  reduce-unsplit-*                  k_loss_reduce, one block per (n, c): 143 pixels (< one stride) and 300 (two strides, ragged end)
  reduce-split-*                    k_loss_reduce on nsplit slabs + k_loss_combine (48 x 48: 2 slabs; C = 4 at 63 x 65: 3, under the size cut)
  reduce-c4-*                       k_loss_reduce_c4 + k_loss_combine (3 x 4 x 64 x 65: 4 slabs, 4160 pixels = 4 x 1024 + 64)
  chain-*-<layout>-<mode>           k_loss_prepare, k_loss_finalize x 4 modes (gsum2 inside and supplied), k_loss_grad x 3 gmodes on the
                                    scalar loop (C = 1, 3, 7), the 16-byte form (ld 4; ld 8 off 4; y = NULL) and the mixed forms (p at
                                    offset 3 of 7-float pixels with y, g aligned: production; g in a 7-float slice), and k_loss_fused
                                    held bit for bit to the staged chain; -2ranks: each half on its own with Bglobal = 2N
  fused-remainder                   k_loss_fused on 25 slabs: one unrolled group of 16 and a remainder loop of 9
  grad-multitrip                    k_loss_grad beyond 8192 x 256 pixels: a second trip of the grid-stride loop
  adam-*                            k_adam<false,false>, <true,false>, <false,true>: float4 body, tail, and a second grid trip
  pad8-*                            k_pad8_bf16<true> (8-float aligned pixels) and <false> (scalar loads)"""
import math

import pytest
import torch

from tests import lossopt_util as U
from tests.normact_util import worst_ratio

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ids = lambda cs: [c.name for c in cs]


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _ok(rc, what):
    assert rc == 0, (what, rc)


def _in(x, case, pad, off):
    """Guarded view holding the (N, HW, C) tensor x: pixel stride C + pad, channel offset off."""
    from tests import guard_util as G
    N, HW, C = x.shape
    return G.view_from(x.reshape(N, case.H, case.W, C).permute(0, 3, 1, 2), ld=C + pad, off=off)[0]


def _read(v):
    from tests import guard_util as G
    return G.read_nchw(v).permute(0, 2, 3, 1).reshape(v.N, v.H * v.W, v.C).cpu()


def _ptr(v):
    return (v.ptr(), v.ld) if v is not None else (None, 0)


def _report(name, ratios):
    print(f'ratio {name} ' + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items()))


# ---- reduction -----------------------------------------------------------------------------------------------------------------------

def _reduce(lib, case, p, y, pad, off, parts):
    """pg_loss_reduce (parts: pg_loss_reduce_parts, its slabs added on the host) -> S (N, C, 5) float64 on the host."""
    N, HW, C = p.shape
    vp, vy = _in(p, case, pad, off), (_in(y, case, pad, off) if U.tconst_of(case) is None else None)
    nd = int(lib.pg_loss_reduce_doubles(N, HW, C))
    assert nd == N * C * 5 * (1 + case.nsplit if case.nsplit > 1 else 1)
    S = torch.full((nd,), float('nan'), dtype=torch.float64, device=DEV)
    args = (vp.ptr(), vp.ld, *_ptr(vy), U.tconst_of(case) or 0.0, N, HW, C, S.data_ptr(), None)
    if parts:
        assert lib.pg_loss_reduce_parts(*args) == case.nsplit
        torch.cuda.synchronize()
        return S[:case.nsplit * N * C * 5].view(case.nsplit, N, C, 5).sum(0).cpu()
    _ok(lib.pg_loss_reduce(*args), 'pg_loss_reduce')
    torch.cuda.synchronize()
    return S[:N * C * 5].view(N, C, 5).cpu()


@pytest.mark.parametrize('case', U.reduce_cases(), ids=['reduce-' + n for n in ids(U.reduce_cases())])
def test_reduce_and_combine(case):
    """All five sums per (n, c), dense and on slices (ld = C + 3, off = 1), from pg_loss_reduce (with k_loss_combine where split)
    and from the slabs of pg_loss_reduce_parts."""
    lib = _lib()
    p, y = U.loss_inputs(case)
    S, A = U.sums_ref(p, y)
    tol = U.tol_sums(A, case.H * case.W)
    r = {}
    for lay, (pad, off) in (('dense', (0, 0)), ('slice', (3, 1))):
        for parts in (False, True):
            r[f'{lay}-{"parts" if parts else "combined"}'] = worst_ratio(_reduce(lib, case, p, y, pad, off, parts), S, tol)
    _report(case.name, r)
    assert max(r.values()) <= 1.0, r


# ---- prepare, finalize, gradient, and the one-launch form ----------------------------------------------------------------------------------

def _stage1(lib, case, lay, p, y):
    N, HW, C = p.shape
    L = U.GRAD_LAYOUTS[lay]
    vp = _in(p, case, *L['p'])
    vy = _in(y, case, *L['y']) if (L['y'] is not None and U.tconst_of(case) is None) else None
    nd = int(lib.pg_loss_reduce_doubles(N, HW, C))
    S = torch.full((nd,), float('nan'), dtype=torch.float64, device=DEV)
    sums = torch.full((2,), float('nan'), dtype=torch.float64, device=DEV)
    tc = U.tconst_of(case) or 0.0
    _ok(lib.pg_loss_reduce(vp.ptr(), vp.ld, *_ptr(vy), tc, N, HW, C, S.data_ptr(), None), 'pg_loss_reduce')
    _ok(lib.pg_loss_prepare(S.data_ptr(), N, C, U.BETA, sums.data_ptr(), None), 'pg_loss_prepare')
    torch.cuda.synchronize()
    return dict(vp=vp, vy=vy, S=S, sums=sums, tc=tc, nd=nd)


def _g_view(case, lay):
    from tests import guard_util as G
    pad, off = U.GRAD_LAYOUTS[lay]['g']
    return G.view(case.N, case.H, case.W, case.C, ld=case.C + pad, off=off)


def _stage2(lib, case, mode, lay, ctx, gsum2, Bglobal):
    """pg_loss_finalize + pg_loss_grad: dict of host tensors (loss, coef, g) and the guard of g."""
    N, HW, C = case.N, case.H * case.W, case.C
    coef = torch.full((N * C * 2,), float('nan'), device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    vg, guard = _g_view(case, lay)
    vp, vy = ctx['vp'], ctx['vy']
    _ok(lib.pg_loss_finalize(ctx['S'].data_ptr(), gsum2.data_ptr() if gsum2 is not None else None, U.MODE_CODE[mode], N, C, HW, Bglobal,
                             U.ALPHA[mode], U.BETA, U.GAMMA, coef.data_ptr(), loss.data_ptr(), None), 'pg_loss_finalize')
    _ok(lib.pg_loss_grad(vp.ptr(), vp.ld, *_ptr(vy), ctx['tc'], coef.data_ptr(), vg.ptr(), vg.ld, N, HW, C, U.GMODE[mode], None), 'pg_loss_grad')
    torch.cuda.synchronize()
    return dict(loss=loss.cpu()[0], coef=coef.cpu().view(N, C, 2), g=_read(vg).float(), guard=guard)


def _fused(lib, case, mode, lay, ctx, gsum2, Bglobal):
    """pg_loss_reduce_parts + pg_loss_value_grad on the same views: (nsplit, loss, S_out, g)."""
    from tests import guard_util as G
    N, HW, C = case.N, case.H * case.W, case.C
    vp, vy = ctx['vp'], ctx['vy']
    S2 = torch.full((ctx['nd'],), float('nan'), dtype=torch.float64, device=DEV)
    Sout = torch.full((N * C * 5,), float('nan'), dtype=torch.float64, device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    vg, guard = _g_view(case, lay)
    ns = lib.pg_loss_reduce_parts(vp.ptr(), vp.ld, *_ptr(vy), ctx['tc'], N, HW, C, S2.data_ptr(), None)
    assert ns == case.nsplit
    _ok(lib.pg_loss_value_grad(S2.data_ptr(), ns, Sout.data_ptr(), gsum2.data_ptr() if gsum2 is not None else None, U.MODE_CODE[mode], N, C, HW,
                               Bglobal, U.ALPHA[mode], U.BETA, U.GAMMA, vp.ptr(), vp.ld, *_ptr(vy), ctx['tc'], vg.ptr(), vg.ld, loss.data_ptr(),
                               None), 'pg_loss_value_grad')
    torch.cuda.synchronize()
    G.assert_untouched(guard, 'slice', 'pg_loss_value_grad g')
    return loss.cpu()[0], Sout.cpu().view(N, C, 5), _read(vg).float()


def _run_chain(lib, case, mode, lay, fused=True):
    """The staged chain of every rank (and, one rank: gsum2 inside against supplied, the one-launch form against staged, bit for
    bit); returns the per-rank results chain_ratios takes."""
    from tests import guard_util as G
    p, y = U.loss_inputs(case)
    N, B = case.N, case.ranks * case.N
    ctxs = [_stage1(lib, case, lay, p[r * N:(r + 1) * N], y[r * N:(r + 1) * N]) for r in range(case.ranks)]
    gsum2 = sum(c['sums'] for c in ctxs)
    got = []
    for ctx in ctxs:
        res = _stage2(lib, case, mode, lay, ctx, gsum2, B)
        G.assert_untouched(res['guard'], 'slice', 'pg_loss_grad g')
        res.update(S=ctx['S'][:N * case.C * 5].view(N, case.C, 5).cpu(), sums=ctx['sums'].cpu())
        if case.ranks == 1:
            inside = _stage2(lib, case, mode, lay, ctx, None, B)
            assert all(torch.equal(inside[k], res[k]) for k in ('loss', 'coef', 'g')), 'gsum2 computed inside differs from supplied'
        if fused:
            for gs in ((gsum2, None) if case.ranks == 1 else (gsum2,)):
                loss, Sout, g = _fused(lib, case, mode, lay, ctx, gs, B)
                assert torch.equal(loss, res['loss']) and torch.equal(Sout, res['S']) and torch.equal(g, res['g']), 'one-launch form differs'
        got.append(res)
    return got


CHAIN = U.chain_cases()


@pytest.mark.parametrize('mode', U.MODES)
@pytest.mark.parametrize('case,lay', CHAIN, ids=[f'{c.name}-{lay}' for c, lay in CHAIN])
def test_prepare_finalize_grad_and_fused(case, lay, mode):
    lib = _lib()
    assert U.loss_nsplit(case.N, case.H * case.W, case.C) == (case.nsplit, case.kernel == 'c4')
    r = U.chain_ratios(case, mode, _run_chain(lib, case, mode, lay))
    _report(f'{case.name}-{lay}-{mode}', r)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('mode', ['tversky', 'bce'])
def test_fused_remainder_slabs(mode):
    """N = 10, C = 1, 160 x 160: nsplit = 25, the unrolled 16-slab loop of k_loss_fused and its remainder loop in one call."""
    lib, case = _lib(), U.FUSED_REMAINDER
    assert case.nsplit == 25
    r = U.chain_ratios(case, mode, _run_chain(lib, case, mode, 'scalar'))
    _report(f'{case.name}-{mode}', r)
    assert max(r.values()) <= 1.0, r


def test_grad_multitrip():
    """BCE, C = 1, N = 33, 256 x 256 against the constant target: 2 162 688 pixels > 8192 x 256 threads."""
    lib, case = _lib(), U.MULTITRIP
    assert case.N * case.H * case.W > 8192 * 256
    r = U.chain_ratios(case, 'bce', _run_chain(lib, case, 'bce', 'vector-ynull', fused=False))
    _report(case.name, r)
    assert max(r.values()) <= 1.0, r


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------

def _adam_call(lib, case, form):
    """One step of pg_adam_step ('arg'), pg_adam_step_dev ('dev') or pg_adam_ema_step ('ema') on the case's state: (p', m', v') on the host."""
    n = case.n
    p, g, m, v = (x.float().to(DEV) for x in U.adam_inputs(case))
    assert all(x.data_ptr() % 16 == 0 for x in (p, g, m, v))
    bc1, sbc2 = 1.0 - U.B1 ** case.t, math.sqrt(1.0 - U.B2 ** case.t)
    if form == 'arg':
        rc = lib.pg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, case.lr, U.B1, U.B2, U.ADAM_EPS, bc1, sbc2, None)
    elif form == 'dev':
        sc = torch.tensor(U.adam_scalars(case.t, case.lr)[3:], dtype=torch.float32, device=DEV)
        rc = lib.pg_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, U.B1, U.B2, U.ADAM_EPS, sc.data_ptr(), None)
    else:
        e = p.clone()
        rc = lib.pg_adam_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, case.lr, U.B1, U.B2, U.ADAM_EPS, bc1,
                                  sbc2, 0.999, None)
    _ok(rc, form)
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu()


def _adam_check(lib, case):
    ref, tol = U.adam_ref(U.adam_inputs(case), U.adam_scalars(case.t, case.lr))
    got = _adam_call(lib, case, 'arg')
    for form in ('dev', 'ema'):
        other = _adam_call(lib, case, form)
        assert all(torch.equal(a, b) for a, b in zip(got, other)), f'{form} differs from pg_adam_step'
    return U.adam_ratios(got, ref, tol)


@pytest.mark.parametrize('n', U.ADAM_NS, ids=[f'adam-single-trip-n{n}' for n in U.ADAM_NS])
def test_adam_step(n):
    """m', v', p' per element after one step, for t in {1, 2, 1000, 100000}, lr in {1e-3, 2e-4}, zero and carried moments; the device-scalar
    and the EMA instantiation bit-identical to pg_adam_step."""
    lib = _lib()
    worst = {}
    for case in U.adam_cases():
        if case.n == n:
            for k, v in _adam_check(lib, case).items():
                worst[k] = max(worst.get(k, 0.0), v)
    _report(f'adam n={n}', worst)
    assert max(worst.values()) <= 1.0, worst


def test_adam_multitrip():
    """n = 8 388 608 + 1027: the float4 body takes a second trip of the grid-stride loop (256 float4s and a ragged end), then 3 tail
    elements."""
    lib, case = _lib(), U.ADAM_BIG
    assert case.n // 4 > 8192 * 256 and case.n % 4 == 3
    r = _adam_check(lib, case)
    _report(f'adam-multitrip n={case.n}', r)
    assert max(r.values()) <= 1.0, r


# ---- pg_pad8_bf16 -------------------------------------------------------------------------------------------------------------------------

def _pad(lib, src_bits, C, aligned):
    from tests import guard_util as G
    npix = src_bits.shape[0]
    if aligned:
        buf = src_bits.to(DEV).contiguous()
        ptr, ld = buf.data_ptr(), 8
        assert ptr % 16 == 0
    else:                                                     # the same values at ld = 9, off = 1: scalar loads
        buf = torch.full((npix, 9), 3.5, device=DEV).view(torch.int32)
        buf[:, 1:1 + C] = src_bits[:, :C].to(DEV)
        ptr, ld = buf.data_ptr() + 4, 9
    dst = G.flat(npix * 16)
    _ok(lib.pg_pad8_bf16(ptr, ld, dst.ptr(), npix, C, None), 'pg_pad8_bf16')
    torch.cuda.synchronize()
    G.assert_untouched(dst, 'all', 'pg_pad8_bf16 dst')
    return dst.inner(torch.int16).cpu().to(torch.int32).view(npix, 8) & 0xFFFF


@pytest.mark.parametrize('npix', U.PAD_NPIX, ids=[f'npix{n}' for n in U.PAD_NPIX])
@pytest.mark.parametrize('C', U.PAD_CS, ids=[f'pad8-aligned-and-scalar-C{c}' for c in U.PAD_CS])
def test_pad8_aligned_and_scalar(C, npix):
    """k_pad8_bf16<true> on 8-float aligned pixels whose channels >= C hold live data, k_pad8_bf16<false> on the same values: bf16 ties
    of both parities and their fp32 neighbours, +-0, the largest float, +-inf, NaN, subnormals -- round-to-nearest-even bit for bit."""
    lib = _lib()
    src, want, sub, nan = U.pad_inputs(npix, C)
    al, sc = _pad(lib, src, C, True), _pad(lib, src, C, False)
    bad = {'aligned': U.pad_mismatches(al, want, sub, nan), 'scalar': U.pad_mismatches(sc, want, sub, nan),
           'forms differ': int((al != sc).sum()), 'subnormals flushed': int((sub & (al != want)).sum())}
    print(f'pad8 C={C} npix={npix} {bad}')
    assert bad['aligned'] == 0 and bad['scalar'] == 0 and bad['forms differ'] == 0, bad
