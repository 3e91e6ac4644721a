"""Every kernel variant of norm_act.hip against float64, per element, with the dropout mask from a NumPy port of the generator.

Calls go through the C ABI (patchgan_amd._lib) on guarded views (tests/guard_util.py: outputs and the unused channels of every
pixel are all-ones NaN, so an element a kernel fails to write, or a neighbour it reads, fails the comparison).  Variants are selected
by shape, alignment, ld, storage type and workspace alone.  References, tolerances, inputs and the case table live in
tests/normact_util.py; tests/test_normact_cpu.py shows without a GPU that they accept a correct fp32 evaluation, reject the
seeded mutations, and that each case takes the path named here (plan numbers from the host-side mirror of pick_group / chunk_plan;
the library's workspace query is held to the mirror below).  Every test prints its worst |got - ref| / tol.

InstanceNorm cases (N x C x H x W; every case: leaky and tanh, p in {0, 0.2}, g2 absent and present, forward then backward;
* = all five activations).  Layouts: al = 16-byte-aligned slice, ld = C + 4 (fp32) / C + 8 (bf16); ld4 = bf16 with ld % 8 == 4;
mis = off 1, ld = C + 3.  fwd / bwd name k_instnorm_fwd / k_instnorm_bwd, P / A name k_in_partial / k_in_apply <VEC, BWD, KD, HG2>;
the chunked cases also run k_in_merge<false> and <true>.

  case                     kernels                                               plan
  3x6x5x7 *  mis           fwd<1>, bwd<1>                                        G 1, 35 pixels
  2x8x1x2                  fwd<4>, bwd<4>                                        HW = 2
  2x8x4x4  (p 0.5 too)     fwd<4>, bwd<4>                                        G 1
  2x8x4x4-mis              fwd<1>, bwd<1> on C % 4 == 0                          G 1
  16x520x3x3               fwd<4>, bwd<4>                                        G 4, 33 groups, the last with 2 of 4 units
  16x130x3x3  mis          fwd<1>, bwd<1>                                        G 4, 33 groups, the last with 2 of 4 units
  2x8x16x32 *              P/A<4,f,0>, P/A<4,t,0,f|t>, fixed                     G 2, 2 chunks of 256, 2 pixels per lane
  2x16x16x32-bf16          P/A<8,f>, P/A<8,t,-1,f|t>, fixed                      G 2, 2 chunks
  2x64x23x23 (-bf16)       as the two above                                      G 16 (8), 16 (8) chunks of 34 (67), last one 19 (60)
  2x24x23x23 (-bf16)       the same kernels, flat form of A (6 / 3 units)        G 4 (2), 2 groups, the last overhanging, 4 (2) chunks
  2x6x23x23  mis           P/A<1,f,0>, P/A<1,t,0,f|t>, flat                      G 4, 2 groups, 4 chunks
  2x6x23x23-bf16  mis      P/A<1,f,-1>, P/A<1,t,-1,f|t>, flat                    the same plan
  2x2x23x23  mis           P/A<1,...,0,...>, fixed                               G 2, 2 chunks
  2x64x23x23-nows          fwd<4>, bwd<4> on 529 pixels (ws = NULL)              G 1
  <shape>-bf16ld4          fwd/bwd<4> or P/A<4,f,-1>, P/A<4,t,-1,f|t>            run-time storage type, all tensors bf16
  <shape>-y32_out16        forward <..,-1> with a bf16 out; backward <..,0,..>   for shapes 2x8x4x4, 2x8x16x32, 2x64x23x23, 2x24x23x23
  <shape>-g16_y32_dy32     forward <..,0>; backward <..,-1,..> with bf16 g1, g2
  <shape>-off100, -off-3   2x8x16x32 and 2x24x23x23 at offset 100 / scale 1 and offset -3 / scale 0.01
  8x256x64x66              P<4,f,0>, P<4,t,0,t>: unrolled main loop              G 64, 128 chunks of 33, 8.25 pixels per lane
  8x256x64x66-bf16         P<8,f>, P<8,t,-1,t>: unrolled main loop               G 32, 128 chunks of 33, 4.125 pixels per lane
  8x256x64x66-mis          P<1,f,0>, P<1,t,0,t>: unrolled main loop              G 64, 4 groups, 32 chunks of 132, 33 pixels per lane
  (the three 8x256x64x66 runs: leaky, p = 0.2, g2 present; one set of bf16-representable inputs and one float64 reference)

Not reachable at test size: the 64-bit index arithmetic beyond 2^31 elements, k_in_apply's flat form beyond 2^31 HW * units, more
than 1024 chunks, N > 65535 (refused)."""
import functools

import pytest
import torch

from tests import normact_util as U

pytestmark = pytest.mark.gpu
PG_OK = 0


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


def _geom(x):
    """(N, H, W, C) of an (N, HW, C) or (npix, C) tensor: the pixels of a sample as one row."""
    return (x.shape[0], 1, x.shape[1], x.shape[2]) if x.dim() == 3 else (1, 1, x.shape[0], x.shape[1])


def _in(x, layout, bf):
    """Guarded view holding x ((N, HW, C) or (npix, C), float64 values representable in the storage type)."""
    from tests import guard_util as G
    N, H, W, C = _geom(x)
    pad, off = U.LAYOUT[layout][bf]
    v, g = G.view_from(x.reshape(N, H, W, C).permute(0, 3, 1, 2), ld=C + pad, off=off, bf=bf)
    return v


def _out(like, layout, bf):
    from tests import guard_util as G
    N, H, W, C = _geom(like)
    pad, off = U.LAYOUT[layout][bf]
    v, g = G.view(N, H, W, C, ld=C + pad, off=off, bf=bf)
    return v


def _read(v, like):
    from tests import guard_util as G
    return G.read_nchw(v).permute(0, 2, 3, 1).reshape(like.shape).cpu()


def _report(family, name, ratios):
    for k, v in ratios.items():
        print(f'ratio {family} {k} {name} {v:.4f}')


def _assert_all(results):
    bad = {k: v for k, v in results.items() if not max(v.values()) <= 1.0}
    assert not bad, bad


# ---- the mask -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('seed', U.SEEDS, ids=hex)
def test_dropout_mask_is_the_port_bit_for_bit(seed, p):
    n = 100003
    m = torch.full((n,), float('nan'), device='cuda')
    assert _lib().pg_dropout_mask(m.data_ptr(), n, p, seed, None) == PG_OK
    torch.cuda.synchronize()
    want = torch.from_numpy(U.keep_mask(seed, n, p)).float()
    assert torch.equal(m.cpu(), want), int((m.cpu() != want).sum())


# ---- InstanceNorm -------------------------------------------------------------------------------------------------------------------

def _norm_call(lib, case, vy, vg1, vg2, ws, ws_bytes, like, act, p, g2on, seed):
    """Forward then backward of one (act, p, g2) of a case: (out, stats, dy) read back as float64 / fp32 on the host."""
    N, C, H, W = case.shape
    HW = H * W
    by, bo, bg, bd = U.MIX[case.mix]
    code = U.ACT_CODE[act]
    vo, vd = _out(like, case.layout, bo), _out(like, case.layout, bd)
    stats = torch.full((N * C * 2,), float('nan'), device='cuda')
    wp = ws.data_ptr() if ws is not None else None
    g2p, g2ld = (vg2.ptr(), vg2.ld) if g2on else (None, 0)
    if case.mix == 'fp32':
        rc = lib.pg_instnorm_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, stats.data_ptr(), N, HW, C, code, 1e-5, p, seed, wp, ws_bytes, None)
    else:
        rc = lib.pg_instnorm_act_fwd_t(vy.ptr(), vy.ld, vo.ptr(), vo.ld, stats.data_ptr(), N, HW, C, code, 1e-5, p, seed, wp, ws_bytes, None,
                                       (1 if by else 0) | (2 if bo else 0))
    assert rc == PG_OK
    torch.cuda.synchronize()
    st = stats.cpu().view(N, C, 2)
    if case.mix == 'fp32':
        rc = lib.pg_instnorm_act_bwd(vg1.ptr(), vg1.ld, g2p, g2ld, vy.ptr(), vy.ld, stats.data_ptr(), vd.ptr(), vd.ld, N, HW, C, code, p, seed,
                                     wp, ws_bytes, None)
    else:
        rc = lib.pg_instnorm_act_bwd_t(vg1.ptr(), vg1.ld, g2p, g2ld, vy.ptr(), vy.ld, stats.data_ptr(), vd.ptr(), vd.ld, N, HW, C, code, p, seed,
                                       wp, ws_bytes, None, (3 if bg else 0) | (4 if by else 0) | (8 if bd else 0))
    assert rc == PG_OK
    torch.cuda.synchronize()
    assert torch.equal(stats.cpu().view(N, C, 2), st)               # the backward reads the statistics and leaves them alone
    return _read(vo, like), st, _read(vd, like)


def _norm_setup(case, y, g1, g2):
    lib = _lib()
    N, C, H, W = case.shape
    by, bo, bg, bd = U.MIX[case.mix]
    full = int(lib.pg_instnorm_workspace_bytes(N, H * W, C))
    assert full == U.workspace_bytes(N, H * W, C)                   # the plan mirror of normact_util is the library's
    ws = torch.empty(max(full, 256), dtype=torch.uint8, device='cuda') if case.ws else None
    return lib, _in(y, case.layout, by), _in(g1, case.layout, bg), _in(g2, case.layout, bg), ws, full if case.ws else 0


SMALL = [c for c in U.norm_cases() if not c.large]
LARGE = [c for c in U.norm_cases() if c.large]


@pytest.mark.parametrize('case', SMALL, ids=[c.name for c in SMALL])
def test_instnorm(case):
    y, g1, g2, frac, left = U.norm_inputs(case)
    lib, vy, vg1, vg2, ws, ws_bytes = _norm_setup(case, y, g1, g2)
    seed = U.seed_of(case)
    results = {}
    for act, p, g2on in U.combos(case):
        out, st, dy = _norm_call(lib, case, vy, vg1, vg2, ws, ws_bytes, y, act, p, g2on, seed)
        h2 = g2 if g2on else None
        ref = U.norm_ref(y, g1, h2, act, p, seed)
        plain = U.plain_norm(y, g1, h2, act, p, seed)
        results[act, p, g2on] = U.norm_ratios(case, ref, plain[2], out, st, dy)
    worst = {k: max(r[k] for r in results.values()) for k in ('fwd', 'mean', 'rstd', 'bwd')}
    _report('norm', case.name, worst)
    _assert_all(results)


@functools.lru_cache(maxsize=None)
def _large_reference():
    """Inputs (bf16-representable, so that all three runs can store them), float64 reference and plain fp32 backward of the
    8.65 M-element case, computed once."""
    case = [c for c in LARGE if c.mix == 'bf16'][0]
    y, g1, g2, frac, left = U.norm_inputs(case)
    assert left == 0 and frac <= 0.01
    act, p, g2on = U.combos(case)[0]
    seed = U.seed_of(case)
    ref = U.norm_ref(y, g1, g2, act, p, seed)
    plain_dy = U.plain_norm(y, g1, g2, act, p, seed)[2]
    return y, g1, g2, act, p, seed, ref, plain_dy


@pytest.fixture(scope='module', autouse=True)
def _drop_large_reference():
    yield
    _large_reference.cache_clear()              # (about 1 GB of float64 tensors)


@pytest.mark.parametrize('case', LARGE, ids=[c.name for c in LARGE])
def test_instnorm_unrolled_main_loops(case):
    y, g1, g2, act, p, seed, ref, plain_dy = _large_reference()
    assert U.combos(case) == [(act, p, True)] and U.norm_plan(case)['ppl'] >= 4
    lib, vy, vg1, vg2, ws, ws_bytes = _norm_setup(case, y, g1, g2)
    out, st, dy = _norm_call(lib, case, vy, vg1, vg2, ws, ws_bytes, y, act, p, True, seed)
    r = U.norm_ratios(case, ref, plain_dy, out, st, dy)
    _report('norm', case.name, r)
    _assert_all({case.name: r})


@pytest.mark.parametrize('case', U.const_cases(), ids=[c.name for c in U.const_cases()])
def test_instnorm_constant_channel(case):
    """A channel of constant 1.5: out exactly 0 (none, leaky, tanh; with and without dropout), rstd = 1 / sqrt(eps) within the
    statistics bound, backward within tolerance for none and tanh (LeakyReLU's derivative at z = 0 exactly is either side's)."""
    y, g1, g2, _, _ = U.norm_inputs(case)
    lib, vy, vg1, vg2, ws, ws_bytes = _norm_setup(case, y, g1, g2)
    seed = U.seed_of(case)
    c = case.const_ch
    results = {}
    for act, p, g2on in U.combos(case):
        out, st, dy = _norm_call(lib, case, vy, vg1, vg2, ws, ws_bytes, y, act, p, g2on, seed)
        assert bool((out[..., c] == 0).all()), (act, p)
        h2 = g2 if g2on else None
        ref = U.norm_ref(y, g1, h2, act, p, seed)
        assert float((ref['rstd'][..., c] - 1e-5 ** -0.5).abs().max()) < 1e-4
        plain = U.plain_norm(y, g1, h2, act, p, seed)
        results[act, p, g2on] = U.norm_ratios(case, ref, plain[2], out, st, dy if act != 'leaky' else None)
    worst = {k: max(r.get(k, 0.0) for r in results.values()) for k in ('fwd', 'mean', 'rstd', 'bwd')}
    _report('norm', case.name, worst)
    _assert_all(results)


@pytest.mark.parametrize('shape', [(2, 8, 16, 32), (2, 24, 23, 23)], ids=lambda s: 'x'.join(map(str, s)))
def test_instnorm_from_host_partials(shape):
    """pg_instnorm_act_fwd_parts on float64 partial sums over 1, 5 and 33 arbitrary pixel chunks (33: past the merge kernel's block
    of 32): the same tolerances; on dyadic inputs, whose sums are exact, the statistics of the three chunkings are bit-identical."""
    from tests import guard_util as G
    lib = _lib()
    N, C, H, W = shape
    HW = H * W
    case = [c for c in SMALL if c.shape == shape and c.mix == 'fp32' and c.layout == 'al'][0]
    y, g1, g2, _, _ = U.norm_inputs(case)
    seed = U.seed_of(case)
    results = {}
    for name, yy in (('random', y), ('dyadic', U.dyadic_inputs(y.shape))):
        vy = _in(yy, 'al', False)
        seen = []
        for chunks in (1, 5, 33):
            part = U.host_partials(yy, U.chunk_bounds(HW, chunks)).cuda()
            for p in (0.0, 0.2):
                vo = _out(yy, 'al', False)
                stats = torch.full((N * C * 2,), float('nan'), device='cuda')
                rc = lib.pg_instnorm_act_fwd_parts(vy.ptr(), vy.ld, vo.ptr(), vo.ld, stats.data_ptr(), part.data_ptr(), chunks, N, HW, C,
                                                   U.ACT_CODE['leaky'], 1e-5, p, seed, None)
                assert rc == PG_OK
                torch.cuda.synchronize()
                st = stats.cpu().view(N, C, 2)
                if name == 'random':            # (the dyadic inputs sit on the knife edge wherever y equals the mean)
                    ref = U.norm_ref(yy, None, None, 'leaky', p, seed)
                    results[chunks, p] = U.norm_ratios(case, ref, None, _read(vo, yy), st, None)
                else:
                    seen.append(st)
        if name == 'dyadic':
            assert all(torch.equal(s, seen[0]) for s in seen)
            ref = U.norm_ref(yy, None, None, 'none', 0.0, seed)
            results['dyadic'] = dict(zip(('mean', 'rstd'), U.stats_ratio(seen[0].double(), ref)))
    _report('parts', 'x'.join(map(str, shape)), {k: max(r.get(k, 0.0) for r in results.values()) for k in ('fwd', 'mean', 'rstd')})
    _assert_all(results)


# ---- plain activation ---------------------------------------------------------------------------------------------------------------

def _act_pair(lib, y, g1, g2, layout, bf, act, p, g2on, seed, with_a=True):
    """pg_act_fwd(_t) on y, then pg_act_bwd(_t) on an `a` that holds the REFERENCE's stored post-dropout output (the backward is
    judged on its own input, not on the forward kernel's result).  Returns the two worst ratios."""
    code = U.ACT_CODE[act]
    npix, C = y.shape
    ref = U.act_ref(y, act, p, seed)
    vy, vo = _in(y, layout, bf), _out(y, layout, bf)
    if bf:
        rc = lib.pg_act_fwd_t(vy.ptr(), vy.ld, vo.ptr(), vo.ld, npix, C, code, p, seed, None, 3)
    else:
        rc = lib.pg_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, npix, C, code, p, seed, None)
    assert rc == PG_OK
    torch.cuda.synchronize()
    wf = U.worst_ratio(_read(vo, y), ref, U.tol_act_fwd(ref), bf)
    a = U.stored(ref, bf) if with_a else None
    h2 = g2 if g2on else None
    rb = U.act_bwd_ref(g1, h2, a, act, p, seed)
    vg1, vg2, vd = _in(g1, layout, bf), _in(g2, layout, bf), _out(y, layout, bf)
    va = _in(a, layout, bf) if with_a else None
    args = (vg1.ptr(), vg1.ld, vg2.ptr() if g2on else None, vg2.ld if g2on else 0, va.ptr() if with_a else None, va.ld if with_a else 0,
            vd.ptr(), vd.ld, npix, C, code, p, seed, None)
    rc = lib.pg_act_bwd_t(*args, 15) if bf else lib.pg_act_bwd(*args)
    assert rc == PG_OK
    torch.cuda.synchronize()
    wb = U.worst_ratio(_read(vd, y), rb['dy'], U.tol_act_bwd(rb, act, p), bf)
    return dict(fwd=wf, bwd=wb)


@pytest.mark.parametrize('name,C,layout,mix,vec', U.ACT_CASES, ids=[c[0] for c in U.ACT_CASES])
def test_act_fwd_bwd(name, C, layout, mix, vec):
    """k_act_fwd<VEC> / k_act_bwd<VEC>: C3 and C8-mis VEC 1, C12 and C4-bf16ld4 VEC 4, C8-bf16 and C24-bf16 VEC 8; every activation,
    p in {0, 0.2}, g2 absent and present, a = NULL with PG_ACT_NONE; inputs include +-0, +-1e-3, +-20, +-90."""
    lib = _lib()
    bf = mix == 'bf16'
    y, g1, g2 = U.act_inputs(U.ACT_NPIX, C, bf)
    results = {}
    for act in U.ACTS:
        for p in (0.0, 0.2):
            for g2on in (False, True):
                results[act, p, g2on] = _act_pair(lib, y, g1, g2, layout, bf, act, p, g2on, U.SEEDS[1])
    for p in (0.0, 0.2):
        results['a=NULL', p] = _act_pair(lib, y, g1, g2, layout, bf, 'none', p, True, U.SEEDS[2], with_a=False)
    _report('act', name, {k: max(r[k] for r in results.values()) for k in ('fwd', 'bwd')})
    _assert_all(results)


def test_act_grid_stride():
    """C = 3, npix = 700 001: 2 100 003 units, more than 8192 * 256 -- the loops of k_act_fwd<1> / k_act_bwd<1> take a second trip."""
    assert U.ACT_STRIDE_NPIX * 3 > 8192 * 256
    y, g1, g2 = U.act_inputs(U.ACT_STRIDE_NPIX, 3, False)
    r = _act_pair(_lib(), y, g1, g2, 'mis', False, 'tanh', 0.2, True, U.SEEDS[0])
    _report('act', 'grid-stride', r)
    _assert_all({'grid-stride': r})


# ---- softmax ------------------------------------------------------------------------------------------------------------------------

def _softmax_cases():
    for C in U.SOFTMAX_CS:
        if C != 4:
            yield f'C{C}', C, {}
    yield 'C4-aligned', 4, {}
    for t in ('y', 'out', 'g1', 'g2', 'dy'):
        yield f'C4-{t}-misaligned', 4, {t: 'mis'}


@pytest.mark.parametrize('name,C,mis', list(_softmax_cases()), ids=[c[0] for c in _softmax_cases()])
def test_softmax(name, C, mis):
    """k_softmax_fwd / k_softmax_bwd: the scalar form (C = 1, 2, 7, 32), the 16-byte form with every view aligned (C = 4) and with
    each view misaligned in turn; g2 absent and present; planted +-80, +-100 and equal logits.  The backward runs on the
    reference's fp32 output."""
    lib = _lib()
    y, g1, g2 = U.softmax_inputs(C)
    lay = lambda t: mis.get(t, 'al' if C % 4 == 0 else 'mis')
    ref = U.softmax_ref(y)
    vy, vo = _in(y, lay('y'), False), _out(y, lay('out'), False)
    assert lib.pg_softmax_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, y.shape[0], C, None) == PG_OK
    torch.cuda.synchronize()
    r = dict(fwd=U.worst_ratio(_read(vo, y), ref, U.tol_softmax_fwd(y, ref)))
    o = ref.float().double()
    vg1, vg2, vout = _in(g1, lay('g1'), False), _in(g2, lay('g2'), False), _in(o, lay('out'), False)
    for g2on in (False, True):
        vd = _out(y, lay('dy'), False)
        rc = lib.pg_softmax_bwd(vg1.ptr(), vg1.ld, vg2.ptr() if g2on else None, vg2.ld if g2on else 0, vout.ptr(), vout.ld, vd.ptr(), vd.ld,
                                y.shape[0], C, None)
        assert rc == PG_OK
        torch.cuda.synchronize()
        h2 = g2 if g2on else None
        r['bwd_g2' if g2on else 'bwd'] = U.worst_ratio(_read(vd, y), U.softmax_bwd_ref(g1, h2, o), U.tol_softmax_bwd(g1, h2, o))
    _report('softmax', name, r)
    _assert_all({name: r})
