"""Zero-tolerance conv tests: on operands whose fp32 arithmetic is provably exact (tests/exact_util.py) every dyadic kernel path
must return the float64 convolution bit for bit -- `torch.equal(got, want32)`, nothing else.  Any difference is a dropped, doubled
or misplaced term, a wrong edge tile, a split-K slab summed twice or a rounding that is not nearest-even; the relative max-norm
bounds of the other kernel tests (2e-5 .. 2e-2) cannot see those.

Exact class: the direct kernels, the implicit GEMMs (fp32 and bf16 MFMA, every tile, split-K), the small-channel kernels, the
bias-gradient column sums, the bf16-tensor kernels, and the polyphase stride-2 Winograd paths in both GEMM forms.  NOT exact, and
kept out by tuning bits (the guard at the end fails if the planner moves a case onto them): the stride-1 Winograd paths and the
opt-in polyphase tile with output edge 4."""
import os

import pytest
import torch

from patchgan_amd import _lib as L
from tests import exact_util as X
from tests.test_fuzz_gpu import _geoms, _geoms_bf16, _geoms_window
from tests.test_kernels_gpu import GEOMS

pytestmark = pytest.mark.gpu

# paths found to do non-dyadic arithmetic that the analysis in exact_util missed: symbol prefix -> the table entry / source line
# that makes it so.  They keep their tolerance tests.  (Empty: none found.)
NOT_EXACT = {}

ALGOS = {'direct': L.ALGO_DIRECT, 'mfma': L.ALGO_MFMA, 'bf16': L.ALGO_BF16, 'auto': L.ALGO_AUTO}
ACT = {'none': L.ACT_NONE, 'relu': L.ACT_RELU}
FORMS = {'s3': 0, 'fp32': L.TUNE_S3_OFF}       # the polyphase GEMMs: split-bf16 (default) / fp32 MFMA (k_wino_bgemm, k_wino_bgemm_mz)
WINO2_GEOMS = [(3, 26, 30, 64, 32, 2), (4, 32, 32, 128, 64, 2), (3, 36, 44, 96, 40, 2), (16, 16, 16, 256, 128, 2)]     # the first: 75 ragged tiles
WINO2W_GEOMS = [(5, 64, 64, 64, 32, 2), (4, 70, 74, 96, 36, 2)]
BWD_BIG_GEOM = (4, 70, 74, 96, 36, 2)
TILE4 = os.environ.get('PATCHGAN_WINO2_TILE') == '4'
TILE4_REASON = 'PATCHGAN_WINO2_TILE=4: the F(4x4,2x2) tables hold 2/9, the polyphase forward / data gradient is not exact'
BF16_GEOMS = _geoms_bf16(30, 0)[:12]
WINDOW_GEOMS = _geoms_window(14, 0)[:6]


def _auto(geom, forced=0):
    """PG_ALGO_AUTO with the non-dyadic paths kept out: no Winograd at all on stride 1, no F(4x4,2x2) polyphase tile."""
    if geom[5] == 1:
        return L.ALGO_AUTO | L.TUNE_WINO_OFF
    if TILE4:
        return L.ALGO_AUTO | L.TUNE_WINO2_OFF | (forced & (L.TUNE_WINO2W_ALL | L.TUNE_S3_OFF))
    return L.ALGO_AUTO | forced


def _geoms_cases(name):
    return [(g, _auto(g) if name == 'auto' else ALGOS[name]) for g in GEOMS]


def _fuzz_cases():
    return [(g, _auto(g, L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL)) for g in _geoms(40, 0)]


def _wino2_cases(form):
    return [(g, L.ALGO_AUTO | L.TUNE_WINO2_ALL | FORMS[form]) for g in WINO2_GEOMS]


def _wino2w_cases(form):
    return [(g, _auto(g, L.TUNE_WINO2W_ALL | FORMS[form])) for g in WINO2W_GEOMS]


def _bwd_big_case(form):
    return BWD_BIG_GEOM, _auto(BWD_BIG_GEOM, L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL | FORMS[form])


def all_fp32_cases():
    """(geometry, algo bits) of every fp32-tensor launch group of this file (tests/test_exact_cpu.py checks each one's budget)."""
    out = [c for name in ALGOS for c in _geoms_cases(name)] + _fuzz_cases()
    for form in FORMS:
        out += ([] if TILE4 else _wino2_cases(form)) + _wino2w_cases(form) + [_bwd_big_case(form)]
    return out


_PICKED = set()         # kernel symbols of the launches this session really made
_RAN = set()            # ... and the test functions that made them
FP32_TESTS = {'geoms', 'wino2', 'wino2w', 'bwd_big', 'fuzz'}


class _Ref:
    """Operands of one geometry on the GPU and, lazily, the fp32 cast of each float64 reference (after the round-trip check)."""

    def __init__(self, ops):
        c = lambda t: t.cuda() if t is not None else None
        self.cpu = ops
        self.ops = X.Operands(ops.geom, c(ops.big), c(ops.small), c(ops.Wt), c(ops.bias_a), c(ops.bias_b), ops.lsb)
        self._r = {}

    def want(self, op, act='none', bias=True):
        key = (op, bias)
        if key not in self._r:
            r = X.reference64(self.ops, op, 'none', bias)
            self._r[key] = tuple(X.to_fp32_exact(t) for t in r) if op == 2 else X.to_fp32_exact(r)
        r = self._r[key]
        return r.clamp_min(0) if act == 'relu' else r


_REFS = {}


def _ref(geom, keep=False):
    if geom in _REFS:
        return _REFS[geom]
    r = _Ref(X.exact_operands(geom))
    if keep:
        _REFS[geom] = r
    return r


def _same(fails, got, want, what):
    if got.shape != want.shape or not torch.equal(got, want):
        bad = ~(got == want)
        d = (got.double() - want.double()).abs()
        fails.append(f'{what}: {int(bad.sum())} of {got.numel()} differ (NaN: {int(got.isnan().sum())}), max |got - want| = '
                     f'{float(d[~d.isnan()].max()) if (~d.isnan()).any() else float("nan")}, max |want| = {float(want.abs().max())}')


def _run_fp32(fails, geom, algo, ref, picked, stats=None):
    """The three ops of one (geometry, algo) on strided, offset, NaN-filled fp32 views: outputs under `none` and `relu` with integer
    biases, dW and dbias, and the InstanceNorm partial sums wherever the kernel can emit them."""
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view, empty_view, pack, DEV
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    op = E.ConvOp(*geom, algo)
    syms = [op.describe(i)[0] for i in range(3)]
    for i in range(3):
        assert not any(syms[i].startswith(k) for k in NOT_EXACT), (geom, syms[i])
        X.budget_for(ref.cpu, i, syms[i])
    picked.update(syms)
    o = ref.ops
    P = pack(o.Wt)
    vb, vs = to_view(o.big, ld=Cb + 4, off=4), to_view(o.small, ld=Ca + 8, off=4)
    tag = f'{geom} algo {algo:#x}'
    for opcode, vin, call, bias, (Ho, Wo, Co) in ((0, vb, op.big2small, o.bias_a, (Hs, Ws, Ca)), (1, vs, op.small2big, o.bias_b, (Hb, Wb, Cb))):
        for act in ('none', 'relu'):
            out = empty_view(N, Ho, Wo, Co, ld=Co + 8, off=4)
            call(vin, P, 0, bias, 0, out, ACT[act])
            _same(fails, out.to_nchw(), ref.want(opcode, act), f'{tag} op {opcode} {syms[opcode]} {act}')
        y = empty_view(N, Ho, Wo, Co, ld=Co + 8, off=4)
        chunks = op.stats_chunks(opcode, vin, y)
        if chunks:
            part = torch.full((N * chunks * Co * 2,), float('nan'), dtype=torch.float64, device=DEV)
            call(vin, P, 0, None, 0, y, part=part)
            want = ref.want(opcode, bias=False)
            _same(fails, y.to_nchw(), want, f'{tag} op {opcode} {syms[opcode]} with partial sums')
            sums, w64 = part.view(N, chunks, Co, 2).sum(1), want.double()
            _same(fails, sums[..., 0], w64.sum((2, 3)), f'{tag} op {opcode} {syms[opcode]} partial sums')
            _same(fails, sums[..., 1], (w64 * w64).sum((2, 3)), f'{tag} op {opcode} {syms[opcode]} partial sums of squares')
            if stats is not None:
                stats.add(syms[opcode].split('<')[0])
    dP = torch.full((16 * Ca * Cb,), float('nan'), device=DEV)
    db = torch.full((Ca,), float('nan'), device=DEV)
    op.wgrad(vs, vb, dP, 0, db, 0)
    dW, dbias = ref.want(2)
    _same(fails, dP, pack(dW), f'{tag} op 2 {syms[2]} dW')
    _same(fails, db, dbias, f'{tag} op 2 {syms[2]} dbias')
    torch.cuda.synchronize()
    return syms


@pytest.mark.parametrize('name', list(ALGOS))
def test_kernel_geometries_all_ops(name):
    """All 29 GEOMS of test_kernels_gpu.py: direct, fp32 MFMA, bf16 MFMA on fp32 tensors, and what PG_ALGO_AUTO picks."""
    fails, picked, stats = [], set(), set()
    for geom, algo in _geoms_cases(name):
        _run_fp32(fails, geom, algo, _ref(geom, keep=True), picked, stats)
    _PICKED.update(picked)
    _RAN.add('geoms')
    print(f'kernel families exercised ({name}):', sorted({k.split("<")[0] for k in picked}), 'partial sums from:', sorted(stats))
    assert not fails, '\n'.join(fails)


@pytest.mark.skipif(TILE4, reason=TILE4_REASON)
@pytest.mark.parametrize('form', list(FORMS))
def test_polyphase_forward_and_data_gradient(form):
    fails, picked, stats = [], set(), set()
    for geom, algo in _wino2_cases(form):
        syms = _run_fp32(fails, geom, algo, _ref(geom, keep=True), picked, stats)
        want = 'k_wino_bgemm_s3' if form == 's3' else 'k_wino_bgemm'
        assert syms[0].split('<')[0] in (want, want + '_mz') and syms[1].split('<')[0] in (want, want + '_mz'), (geom, syms)
    _PICKED.update(picked)
    _RAN.add('wino2')
    print(f'kernels exercised ({form}):', sorted(picked), 'partial sums from:', sorted(stats))
    assert stats, 'no polyphase launch emitted partial sums'
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('form', list(FORMS))
def test_polyphase_weight_gradient(form):
    fails, picked = [], set()
    for geom, algo in _wino2w_cases(form):
        syms = _run_fp32(fails, geom, algo, _ref(geom, keep=True), picked)
        assert syms[2].split('<')[0] == ('k_wino_wgrad_gemm_s3' if form == 's3' else 'k_wino_wgrad_gemm'), (geom, syms)
    _PICKED.update(picked)
    _RAN.add('wino2w')
    print(f'kernels exercised ({form}):', sorted(picked))
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('form', list(FORMS))
def test_bwd_big_both_outputs(form):
    """pg_conv4x4_bwd_big with both halves forced onto the polyphase paths: dW and the data gradient are both exact."""
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view, empty_view, pack, DEV
    geom, algo = _bwd_big_case(form)
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    ref = _ref(geom, keep=True)
    op = E.ConvOp(*geom, algo)
    syms = [op.describe(i)[0] for i in (0, 2)]
    X.budget_for(ref.cpu, 0, syms[0])
    X.budget_for(ref.cpu, 2, syms[1])
    assert syms[1].startswith('k_wino_wgrad_gemm'), syms
    _PICKED.update(syms)
    _RAN.add('bwd_big')
    o = ref.ops
    vs, vb = to_view(o.small, ld=Ca + 4, off=4), to_view(o.big, ld=Cb + 8, off=4)
    dP = torch.full((16 * Ca * Cb,), float('nan'), device=DEV)
    ds = empty_view(N, Hs, Ws, Ca, ld=Ca + 8, off=4)
    op.bwd_big(vs, vb, pack(o.Wt), dP, 0, ds)
    fails = []
    _same(fails, dP, pack(ref.want(2)[0]), f'bwd_big dW {syms}')
    _same(fails, ds.to_nchw(), ref.want(0, bias=False), f'bwd_big data gradient {syms}')
    assert not fails, '\n'.join(fails)


def test_random_geometries_seed0():
    """The 40 geometries of fuzz seed 0, polyphase paths forced wherever the geometry allows, stride 1 off Winograd."""
    fails, picked, stats = [], set(), set()
    for geom, algo in _fuzz_cases():
        _run_fp32(fails, geom, algo, _ref(geom), picked, stats)
    _PICKED.update(picked)
    _RAN.add('fuzz')
    print('kernel families exercised:', sorted({k.split('<')[0] for k in picked}), 'partial sums from:', sorted(stats))
    assert not fails, '\n'.join(fails)


def _run_bf16(fails, geom, algo, picked, window):
    """bf16 tensors (PG_IO_*) as tests/test_fuzz_gpu.py runs them; fp32 outputs exact, bf16 outputs the nearest-even rounding of the
    exact sum (no ulp of slack: on exact sums round-to-nearest-even is unique), partial sums those of the stored tensor."""
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view_bf, to_view_bf8, empty_view, empty_view_bf, pack, DEV
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    ref = _ref(geom)
    o = ref.ops
    op = E.ConvOp(*geom, algo)
    P = pack(o.Wt)
    few = Cb <= 8
    vb = to_view_bf8(o.big) if few else to_view_bf(o.big, ld=Cb + 8, off=8)
    vs = to_view_bf(o.small, ld=Ca + 8, off=8)
    tag = f'{geom} algo {algo:#x} bf16 tensors'
    n = 0

    def budget(opcode, sym):
        assert sym.startswith(('k_conv_bf16', 'k_wgrad_bf16')), (geom, opcode, sym)
        X.budget_for(ref.cpu, opcode, sym)
        picked.add(sym)

    for opcode, src, call, bias, oshape, ok in ((0, vb, op.big2small, o.bias_a, (N, Hs, Ws, Ca), few or Cb % 64 == 0),
                                                (1, vs, op.small2big, o.bias_b, (N, Hb, Wb, Cb), Ca % 64 == 0)):
        outs = [not (opcode == 1 and few)]                 # small2big onto <= 8 channels writes fp32 (PG_IO_SMALL_BF16 alone)
        if window:
            ok = op.describe(opcode, L.IO_MASK)[0].startswith('k_conv_bf16r')
            outs = [True, False]                           # the window kernel stores either type
        if not ok:
            continue
        cout = oshape[3]
        for out_bf in outs:
            io = L.IO_MASK if out_bf else (L.IO_BIG_BF16 if opcode == 0 else L.IO_SMALL_BF16)
            sym = op.describe(opcode, io)[0]
            budget(opcode, sym)
            for act in ('none', 'relu'):
                got = (empty_view_bf if out_bf else empty_view)(*oshape, ld=cout + 8, off=8)
                call(src, P, 0, bias, 0, got, ACT[act])
                want = ref.want(opcode, act)
                _same(fails, got.to_nchw(), want.bfloat16().float() if out_bf else want, f'{tag} op {opcode} {sym} {act} -> {"bf16" if out_bf else "fp32"}')
                n += 1
        y = empty_view_bf(*oshape, ld=cout + 8, off=8)
        chunks = op.stats_chunks(opcode, src, y) if not (opcode == 1 and few) else 0
        if chunks:
            part = torch.full((N * chunks * cout * 2,), float('nan'), dtype=torch.float64, device=DEV)
            call(src, P, 0, None, 0, y, part=part)
            stored = ref.want(opcode, bias=False).bfloat16().float()
            _same(fails, y.to_nchw(), stored, f'{tag} op {opcode} with partial sums')
            sums, w64 = part.view(N, chunks, cout, 2).sum(1), stored.double()
            _same(fails, sums[..., 0], w64.sum((2, 3)), f'{tag} op {opcode} partial sums')
            _same(fails, sums[..., 1], (w64 * w64).sum((2, 3)), f'{tag} op {opcode} partial sums of squares')
            picked.add('part:' + op.describe(opcode, L.IO_MASK)[0].split('<')[0])
    if not window and Ca % 32 == 0 and Ca >= 64 and (few or Cb % 32 == 0):
        budget(2, op.describe(2, L.IO_MASK)[0])
        dP = torch.full((16 * Ca * Cb,), float('nan'), device=DEV)
        op.wgrad(vs, vb, dP, 0)
        _same(fails, dP, pack(ref.want(2)[0]), f'{tag} op 2 {op.describe(2, L.IO_MASK)[0]} dW')
        n += 1
    torch.cuda.synchronize()
    return n


def _bf16_symbols(picked):
    return (sum(k.startswith(('k_conv_bf16x', 'k_conv_bf16r')) for k in picked), sum(k.startswith('k_wgrad_bf16x') for k in picked))


@pytest.mark.parametrize('staging', ['flat', 'ring'])
def test_bf16_tensors(staging):
    fails, picked = [], set()
    tune = L.TUNE_BF16X_RING if staging == 'ring' else L.TUNE_BF16X_FLAT
    n = sum(_run_bf16(fails, geom, L.ALGO_BF16 | tune, picked, False) for geom in BF16_GEOMS)
    _PICKED.update(picked)
    print(f'bf16 kernels exercised ({staging}, {n} launches):', sorted(picked))
    assert _bf16_symbols(picked)[0] >= 6 and _bf16_symbols(picked)[1] >= 3, sorted(picked)
    assert not fails, '\n'.join(fails)


def test_bf16_window_kernel():
    fails, picked = [], set()
    n = sum(_run_bf16(fails, geom, L.ALGO_BF16, picked, True) for geom in WINDOW_GEOMS)
    _PICKED.update(picked)
    print(f'window kernel launches checked: {n}:', sorted(picked))
    assert n >= 12 and any(k.startswith('part:') for k in picked), (n, sorted(picked))
    assert not fails, '\n'.join(fails)


def test_wide_operands_through_the_split_bf16_gemms():
    """The second and third bf16 pieces: fixed-point operands of up to 16 bits (tests/exact_util.py: wide_*_operands; the CPU test
    shows that each of the six products a_i b_j changes the result of one of them) through k_wino_bgemm_s3 (both directions) and
    k_wino_wgrad_gemm_s3, zero tolerance."""
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view, empty_view, pack, DEV
    fails = []
    for geom in ([] if TILE4 else WINO2_GEOMS):
        N, Hb, Wb, Ca, Cb, s = geom
        Hs, Ws = X.dims(geom)
        op = E.ConvOp(*geom, L.ALGO_AUTO | L.TUNE_WINO2_ALL)
        for opcode in (0, 1):
            sym = op.describe(opcode)[0]
            assert sym.startswith('k_wino_bgemm_s3'), (geom, sym)
            _PICKED.add(sym)
            for shape in X.WIDE:
                ref = _Ref(X.wide_conv_operands(geom, opcode, shape))
                X.wide_budget(ref.cpu, opcode)
                o = ref.ops
                if opcode == 0:
                    out = empty_view(N, Hs, Ws, Ca, ld=Ca + 8, off=4)
                    op.big2small(to_view(o.big, ld=Cb + 4, off=4), pack(o.Wt), 0, None, 0, out)
                else:
                    out = empty_view(N, Hb, Wb, Cb, ld=Cb + 8, off=4)
                    op.small2big(to_view(o.small, ld=Ca + 4, off=4), pack(o.Wt), 0, None, 0, out)
                _same(fails, out.to_nchw(), ref.want(opcode, bias=False), f'{geom} op {opcode} {sym} wide ({shape})')
    for geom in WINO2W_GEOMS:
        N, Hb, Wb, Ca, Cb, s = geom
        op = E.ConvOp(*geom, _auto(geom, L.TUNE_WINO2W_ALL))
        sym = op.describe(2)[0]
        assert sym.startswith('k_wino_wgrad_gemm_s3'), (geom, sym)
        _PICKED.add(sym)
        for shape in X.WIDE:
            ref = _Ref(X.wide_wgrad_operands(geom, shape))
            X.wide_budget(ref.cpu, 2)
            o = ref.ops
            dP = torch.full((16 * Ca * Cb,), float('nan'), device=DEV)
            op.wgrad(to_view(o.small, ld=Ca + 4, off=4), to_view(o.big, ld=Cb + 8, off=4), dP, 0)
            _same(fails, dP, pack(ref.want(2)[0]), f'{geom} op 2 {sym} wide ({shape})')
    torch.cuda.synchronize()
    if TILE4:
        print('forward / data gradient left out:', TILE4_REASON)
    assert not fails, '\n'.join(fails)


def planned_symbols():
    """Kernel symbols of every case list above, from the planner's own answers (the launches go through the same ConvOp)."""
    from patchgan_amd import engine as E
    syms = set()
    for geom, algo in all_fp32_cases():
        if TILE4 and algo & L.TUNE_WINO2_ALL:
            continue
        op = E.ConvOp(*geom, algo)
        syms.update(op.describe(i)[0] for i in range(3))
    return syms


def test_coverage_guard():
    """The fp32-tensor cases reach every family of the exact class and none of the non-dyadic one (a planner change must not silently
    move a layer out of the exact class, or a family out of this file).  The bf16-tensor families are counted in their own tests."""
    syms = planned_symbols()
    fam = {k.split('<')[0] for k in syms}
    print('kernel families exercised:', sorted(fam))
    print('kernels exercised:', sorted(syms))
    need = {'k_wino_wgrad_gemm_s3', 'k_wino_wgrad_gemm', 'k_b2s_tapkp', 'k_s2b_tapnf', 'k_s2b_ca1', 'k_wgrad_tapn'}
    if not TILE4:
        need |= {'k_wino_bgemm_s3', 'k_wino_bgemm'}
    assert need <= fam, sorted(need - fam)
    assert any(k.endswith('+k_col2im_small2big') for k in syms) and any(k.endswith('+k_gather_big2small') for k in syms), sorted(syms)     # the row GEMMs
    assert not any(k.startswith('k_wino_gemm') for k in fam), sorted(fam)
    for geom, algo in all_fp32_cases():
        if geom[5] == 1:
            from patchgan_amd import engine as E
            assert not any(E.ConvOp(*geom, algo).describe(i)[0].startswith('k_wino') for i in range(3)), geom
    ran = {k for k in _PICKED if not k.startswith(('k_conv_bf16', 'k_wgrad_bf16x', 'part:'))}       # (the bf16-tensor kernels aside)
    assert ran <= syms, sorted(ran - syms)          # what ran is what was planned ...
    if _RAN >= FP32_TESTS - ({'wino2'} if TILE4 else set()):
        missing = {k.split('<')[0] for k in syms} - {k.split('<')[0] for k in ran}
        assert not missing, sorted(missing)         # ... and, when the whole file ran, every planned family was launched
