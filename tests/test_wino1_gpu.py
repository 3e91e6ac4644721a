"""The stride-1 Winograd kernels of conv_wino.hip held to float64, element by element (tests/wino1_util.py has the yardstick and the
statistic; tests/test_wino1_cpu.py shows that both discriminate).

Every GEMM form of the forward / data gradient -- F(2x2,4x4) on 64-tile and 128-tile rows, the fused F(3x3,4x4) instance unsliced
and on 2 / 4 K slices with the slab reduce, the row-split pair in its fp32 and split-bf16 forms, both LDS-DMA kernels -- and of the
weight gradient -- F(4x4,2x2) and F(4x4,3x3), 64x64 and 128x128 output tiles, fp32 and split-bf16, K-sliced -- runs at the smallest
geometry that still selects it, on NaN-filled strided offset views, selected by per-call tuning bits and view alignment only:
  dense    e_i = |got_i - ref64_i| / S_i; max e <= 4 x and rms e <= 2 x those of the fp32 model on the same operands and device
  probes   input confined to the last sample's last two rows and columns: every tile whose window misses it returns the bias
           EXACTLY (==), the others meet the same bound; weight gradient: dy confined to the last ragged tile, and dy = 0 -> 0
  fuzz     seeded ragged geometries (the generator of tools/fuzz_stride1.py, size-capped) through the same statistic
  guard    the case lists plan onto every family, and when the whole file ran every planned symbol was launched
The measured figures are printed per kernel symbol (EXPERIMENTS.md keeps the table of one run)."""
import random

import pytest
import torch

from patchgan_amd import _lib as L
from tests import exact_util as X
from tests import wino1_util as W

pytestmark = pytest.mark.gpu

# kernels found to exceed the bound whose fix was out of reach: symbol -> (source line that explains it, measured figures).  They are
# reported, not asserted, and keep their tolerance tests.  (Empty: none found.)
NOT_WITHIN = {}

F2, F3, DMA, S3_OFF = L.TUNE_WINO1_F2, L.TUNE_WINO1_F3, L.TUNE_WINO_DMA, L.TUNE_S3_OFF
K_F2_64, K_F2_128, K_F3 = 'k_wino_gemm<1,1,2,2,4,2>', 'k_wino_gemm<2,1,2,2,2,2>', 'k_wino_gemm<1,1,2,2,2,3>'
K_ROW, K_ROW_S3, K_DMA2, K_DMA3 = 'k_wino_gemm_row<4,1>', 'k_wino_gemm_row_s3<2>', 'k_wino_gemm_dma<2,3,3>', 'k_wino_gemm_dma<3,4,2>'
K_W64, K_W64_S3, K_W128_S3 = 'k_wino_wgrad_gemm<1,1,2,2>', 'k_wino_wgrad_gemm_s3<1,1,2,2,2,3>', 'k_wino_wgrad_gemm_s3<2,2,2,2,1,2>'

# (N, Hb, Wb, Ca, Cb, 1).  pg_wino_geom_ok wants N ceil(Ho/2) ceil(Wo/2) >= 2048: 2 x 33 x 32 = 2112 forward (65 x 64 outputs: ragged
# for F2 in one direction, for F3 in both), 2 x 33 x 33 data gradient (66 x 65)
G64 = (2, 66, 65, 64, 64, 1)


def _f3(slices):
    """The three F(3x3,4x4) forms: (bits, 16-byte-aligned output, symbol, K slices).  An output view pg_wino_gemm_rows refuses (8-byte
    aligned) takes the fully fused kernel, which alone slices K."""
    return [(F3, True, K_ROW_S3, 1), (F3 | S3_OFF, True, K_ROW, 1), (F3, False, K_F3, slices)]


# (geometry, opcode 0 forward / 1 data gradient) -> forms
FWD_CASES = {
    (G64, 0): [(F2, True, K_F2_64, 1), (F2 | DMA, True, K_DMA2, 1), (F3 | DMA, True, K_DMA3, 1)] + _f3(1),
    (G64, 1): [(F2, True, K_F2_64, 1), (F2 | DMA, True, K_DMA2, 1), (F3 | DMA, True, K_DMA3, 1)] + _f3(1),
    ((2, 66, 65, 64, 128, 1), 0): _f3(2),                   # Cin = 128: two K slices + slab reduce
    ((2, 66, 65, 64, 256, 1), 0): _f3(4),                   # Cin = 256: four
    ((2, 66, 65, 128, 64, 1), 1): _f3(2),                   # the same in the data gradient (Cin = Ca)
    ((2, 66, 65, 256, 64, 1), 1): _f3(4),
    ((2, 66, 65, 64, 96, 1), 0): [(F2, True, K_F2_64, 1)],  # Cin = 96: three 32-wide K chunks, F(2x2,4x4) only
    ((2, 66, 65, 64, 96, 1), 1): [(F2, True, K_F2_64, 1)] + _f3(1),      # Cout = 96: a ragged 64-channel tile
    # pg_wino_small_tile false: ceil(T / 128) ceil(Cout / 64) >= 400 at the fewest FLOPs is 16 x 25 (T = 2048 exactly); 1540 channels
    # leave the 25th channel tile ragged
    ((2, 65, 65, 1540, 64, 1), 0): [(F2, True, K_F2_128, 1)],
}
# weight gradient: geometry -> dy tile edge.  r = 3 needs N ceil(Hs/3) ceil(Ws/3) >= 1024: 4 x 16 x 16 on 46 x 47 maps (one / two leftover
# rows / columns); 128-multiples on both sides select the 128 x 128 tile in the split-bf16 form
WGRAD_CASES = {G64: 2, (4, 47, 48, 64, 64, 1): 3, (2, 66, 65, 128, 128, 1): 2, (4, 47, 48, 128, 128, 1): 3}
WGRAD_FORMS = {'s3': 0, 'fp32': S3_OFF}
FUZZ_CASES = 12

_LAUNCHED = set()       # kernel symbols this session really launched
_RAN = set()            # tests that ran to their end
_FIGURES = {}           # symbol -> [(model Stat, kernel Stat)]
ACT = {'none': L.ACT_NONE, 'leakyrelu': L.ACT_LEAKY}


def _ids(key):
    return 'x'.join(map(str, key[0][:5])) + ('-fwd', '-dgrad')[key[1]]


def _launched(op, opcode, aligned=True):
    """The symbol the call will launch: ConvOp.describe plans from the geometry alone; the row-split pair needs a 16-byte-aligned
    output (pg_wino_gemm_rows), any other view takes the fused F(3x3,4x4) kernel."""
    sym = op.describe(opcode)[0]
    return K_F3 if (sym.startswith('k_wino_gemm_row') and not aligned) else sym


def _record(fails, what, sym, k, m):
    line = W.report(f'{sym} {what}', k, m)
    print(line)
    _LAUNCHED.add(sym)
    _FIGURES.setdefault(sym, []).append((m, k))
    if not W.within(k, m) and sym not in NOT_WITHIN:
        fails.append(line)


class _Ctx:
    """Operands of one geometry on the GPU, their views, and lazily the float64 references and fp32 model statistics."""

    def __init__(self, geom, seed=0):
        from tests.gpu_util import to_view, pack, DEV
        self.geom = geom
        N, Hb, Wb, Ca, Cb, s = geom
        self.ops = o = W.normal_operands(geom, seed, DEV)
        self.P = pack(o.Wt)
        self.vb, self.vs = to_view(o.big, ld=Cb + 4, off=4), to_view(o.small, ld=Ca + 8, off=4)
        self.probe = W.replaced(o, big=W.corner_input(o.big), small=W.corner_input(o.small))
        self.pvb, self.pvs = to_view(self.probe.big, ld=Cb + 4, off=4), to_view(self.probe.small, ld=Ca + 8, off=4)
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def ref(self, opcode, act='none', probe=False):
        return self._get(('ref', opcode, act, probe), lambda: W.ref_and_scale(self.probe if probe else self.ops, opcode, act))

    def model(self, opcode, mo, act='none', probe=False):
        """The fp32 model's output of opcode 0 / 1 on tile edge mo."""
        o = self.probe if probe else self.ops
        fn, x, bias = ((W.wino1_fwd_model, o.big, o.bias_a), (W.wino1_dgrad_model, o.small, o.bias_b))[opcode]
        return self._get(('model', opcode, mo, act, probe), lambda: fn(x, o.Wt, mo, torch.float32, bias, act))


_CTX = {}


def _ctx(geom):
    if geom not in _CTX:
        _CTX[geom] = _Ctx(geom)
    return _CTX[geom]


def _call(c, op, opcode, aligned, act, probe=False):
    """One forward / data-gradient launch onto a fresh NaN-filled view; returns the NCHW result."""
    from tests.gpu_util import empty_view
    N, Hb, Wb, Ca, Cb, s = c.geom
    Hs, Ws = X.dims(c.geom)
    off = 4 if aligned else 2
    if opcode == 0:
        out = empty_view(N, Hs, Ws, Ca, ld=Ca + 8, off=off)
        op.big2small(c.pvb if probe else c.vb, c.P, 0, c.ops.bias_a, 0, out, ACT[act])
    else:
        out = empty_view(N, Hb, Wb, Cb, ld=Cb + 8, off=off)
        op.small2big(c.pvs if probe else c.vs, c.P, 0, c.ops.bias_b, 0, out, ACT[act])
    return out.to_nchw()


@pytest.mark.parametrize('key', list(FWD_CASES), ids=_ids)
def test_forward_and_data_gradient_dense(key):
    from patchgan_amd import engine as E
    geom, opcode = key
    c, fails = _ctx(geom), []
    for act in ('none', 'leakyrelu'):
        ref, S = c.ref(opcode, act)
        for bits, aligned, want_sym, _ in FWD_CASES[key]:
            op = E.ConvOp(*geom, L.ALGO_AUTO | bits)
            sym = _launched(op, opcode, aligned)
            assert sym == want_sym, (key, hex(bits), aligned, sym)
            m = W.Stat(c.model(opcode, W.fwd_tile_edge(sym), act), ref, S)
            _record(fails, f'{_ids(key)} {act}', sym, W.Stat(_call(c, op, opcode, aligned, act), ref, S), m)
    torch.cuda.synchronize()
    _RAN.add(('dense', key))
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('key', list(FWD_CASES), ids=_ids)
def test_forward_and_data_gradient_probe(key):
    """Input non-zero only in the last sample's last two rows and columns (the same tensor serves as dy of the data gradient)."""
    from patchgan_amd import engine as E
    geom, opcode = key
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    c, fails = _ctx(geom), []
    ref, S = c.ref(opcode, 'none', probe=True)
    bias = c.ops.bias_a if opcode == 0 else c.ops.bias_b
    H, Wd, pad = (Hb, Wb, 1) if opcode == 0 else (Hs, Ws, 2)
    for bits, aligned, want_sym, _ in FWD_CASES[key]:
        op = E.ConvOp(*geom, L.ALGO_AUTO | bits)
        sym = _launched(op, opcode, aligned)
        assert sym == want_sym, (key, hex(bits), aligned, sym)
        mo = W.fwd_tile_edge(sym)
        quiet = W.quiet_mask(N, H, Wd, pad, mo, ref.device)
        bad_m, m = W.probe_stats(c.model(opcode, mo, 'none', probe=True), ref, S, bias, quiet)
        assert bad_m == 0, 'the model itself leaks into quiet tiles'
        got = _call(c, op, opcode, aligned, 'none', probe=True)
        bad, k = W.probe_stats(got, ref, S, bias, quiet)
        if bad:
            where = ((~(got == bias.view(1, -1, 1, 1))) & quiet[:, None]).nonzero()[:4].tolist()
            fails.append(f'{sym} {_ids(key)}: {bad} elements of quiet tiles differ from their bias (NaN: {int(got.isnan().sum())}), first at {where}')
        _record(fails, f'{_ids(key)} probe ({int((~quiet).sum())} live pixels)', sym, k, m)
    torch.cuda.synchronize()
    _RAN.add(('probe', key))
    assert not fails, '\n'.join(fails)


def _wgrad(op, vs, vb, Ca, Cb, **kw):
    from tests.gpu_util import DEV
    dP = torch.full((16 * Ca * Cb,), float('nan'), device=DEV)
    db = torch.full((Ca,), float('nan'), device=DEV)
    op.wgrad(vs, vb, dP, 0, db, 0, **kw)
    torch.cuda.synchronize()
    return dP.view(4, 4, Ca, Cb).permute(2, 3, 0, 1), db


def _check_dbias(fails, what, db, dy):
    """The bias gradient is a plain column sum of K = N Hs Ws terms, not a Winograd kernel; the workspace it shares with dW is why every
    case passes it.  Any summation order: K - 1 roundings of at most 2^-24 sum|dy| each, independent -> sqrt(K) 2^-24 sum|dy|."""
    d = dy.double()
    K = d.numel() // d.shape[1]
    e = float(((db.double() - d.sum((0, 2, 3))).abs() / d.abs().sum((0, 2, 3))).max())
    print(f'{what} dbias: max e {e:.3e} (bound {K ** 0.5 * 2.0 ** -24:.3e})')
    if not e <= K ** 0.5 * 2.0 ** -24:
        fails.append(f'{what} dbias: max e {e:.3e}')


@pytest.mark.parametrize('form', list(WGRAD_FORMS))
@pytest.mark.parametrize('geom', list(WGRAD_CASES), ids=lambda g: 'x'.join(map(str, g[:5])))
def test_weight_gradient_dense_and_probe(geom, form):
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    r = WGRAD_CASES[geom]
    c, fails = _ctx(geom), []
    op = E.ConvOp(*geom, L.ALGO_AUTO | WGRAD_FORMS[form])
    sym, slices = op.describe(2)
    assert sym == _wgrad_symbol(geom, form) and r == W.wgrad_r(N, Hs, Ws), (geom, form, sym, r)
    tag = f'{"x".join(map(str, geom[:5]))} F(4x4,{r}x{r}) {slices} slices'
    o = c.ops
    # dense
    ref, S = c.ref(2)
    m = W.Stat(c._get(('wmodel', r), lambda: W.wino1_wgrad_model(o.big, o.small, r, torch.float32)), ref, S)
    dW, db = _wgrad(op, c.vs, c.vb, Ca, Cb)
    _record(fails, tag, sym, W.Stat(dW, ref, S), m)
    _check_dbias(fails, tag, db, o.small)
    # dy non-zero only in the last (ragged) tile: the tensor-wide max S normalises
    dy = W.last_tile_dy(o.small, r)
    pops = W.replaced(o, small=dy)
    ref, S = c._get(('wprobe', r), lambda: W.ref_and_scale(pops, 2))
    m = W.Stat(c._get(('wprobe model', r), lambda: W.wino1_wgrad_model(o.big, dy, r, torch.float32)), ref, S, norm=S.max())
    dW, db = _wgrad(op, to_view(dy, ld=Ca + 8, off=4), c.vb, Ca, Cb)
    _record(fails, tag + ' probe', sym, W.Stat(dW, ref, S, norm=S.max()), m)
    _check_dbias(fails, tag + ' probe', db, dy)
    # dy = 0
    dW, db = _wgrad(op, to_view(torch.zeros_like(o.small), ld=Ca + 8, off=4), c.vb, Ca, Cb)
    if not (bool((dW == 0).all()) and bool((db == 0).all())):
        fails.append(f'{sym} {tag}: dy = 0 gives {int((dW != 0).sum())} non-zero dW, {int((db != 0).sum())} non-zero dbias (NaN: {int(dW.isnan().sum())})')
    _RAN.add(('wgrad', geom, form))
    assert not fails, '\n'.join(fails)


def _wgrad_symbol(geom, form):
    if form == 'fp32':
        return K_W64
    return K_W128_S3 if geom[3] % 128 == 0 and geom[4] % 128 == 0 else K_W64_S3


# ---- seeded fuzz ------------------------------------------------------------------------------------------------------------------------
_FUZZ = []


def _fuzz_geoms():
    """The generator of tools/fuzz_stride1.py under the size cap of test_fuzz_gpu._geoms: the first FUZZ_CASES draws whose forward the
    planner puts on a k_wino path."""
    from patchgan_amd import engine as E
    if not _FUZZ:
        rng = random.Random(0)
        for _ in range(2000):
            if len(_FUZZ) == FUZZ_CASES:
                break
            N = rng.choice([4, 6, 9, 12, 16, 24])
            Hb, Wb = rng.randint(24, 72), rng.randint(24, 72)
            Ca, Cb = rng.choice([64, 96, 128, 160, 256, 512]), rng.choice([64, 128, 192, 256])
            bits = rng.choice([0, 0, F2, F3])
            if N * Hb * Wb * max(Ca, Cb) > 6_000_000 or Ca * Cb > 40_000:
                continue
            if E.ConvOp(N, Hb, Wb, Ca, Cb, 1, L.ALGO_AUTO | bits).describe(0)[0].startswith('k_wino'):
                _FUZZ.append(((N, Hb, Wb, Ca, Cb, 1), bits))
    return _FUZZ


@pytest.mark.parametrize('i', range(FUZZ_CASES))
def test_fuzz_against_float64(i):
    """Forward (bias + LeakyReLU, keeping V where the layer's weight gradient takes it), data gradient and weight gradient of one drawn
    geometry: whatever k_wino kernel the planner picks meets the bound."""
    from patchgan_amd import engine as E
    geoms = _fuzz_geoms()
    assert len(geoms) == FUZZ_CASES, len(geoms)
    geom, bits = geoms[i]
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    c, fails = _Ctx(geom, seed=1), []
    op = E.ConvOp(*geom, L.ALGO_AUTO | bits)
    vk = op.keep_v(True, c.vb, c.vs)
    tag = f'fuzz {i} {"x".join(map(str, geom[:5]))} bits {bits:#x}' + (' V kept' if vk is not None else '')
    for opcode, act in ((0, 'leakyrelu'), (1, 'none')):
        sym = _launched(op, opcode)
        if not sym.startswith('k_wino'):
            continue
        ref, S = c.ref(opcode, act)
        m = W.Stat(c.model(opcode, W.fwd_tile_edge(sym), act), ref, S)
        if opcode == 0 and vk is not None:
            from tests.gpu_util import empty_view
            out = empty_view(N, Hs, Ws, Ca, ld=Ca + 8, off=4)
            op.big2small(c.vb, c.P, 0, c.ops.bias_a, 0, out, ACT[act], v_keep=vk)
            got = out.to_nchw()
        else:
            got = _call(c, op, opcode, True, act)
        _record(fails, tag, sym, W.Stat(got, ref, S), m)
    sym = op.describe(2)[0]
    if sym.startswith('k_wino_wgrad'):
        r = W.wgrad_r(N, Hs, Ws)
        ref, S = c.ref(2)
        m = W.Stat(W.wino1_wgrad_model(c.ops.big, c.ops.small, r, torch.float32), ref, S)
        dW, db = _wgrad(op, c.vs, c.vb, Ca, Cb, **({'v_pre': vk} if vk is not None else {}))
        _record(fails, tag + f' F(4x4,{r}x{r})', sym, W.Stat(dW, ref, S), m)
        _check_dbias(fails, tag, db, c.ops.small)
    torch.cuda.synchronize()
    _RAN.add(('fuzz', i))
    assert not fails, '\n'.join(fails)


# ---- coverage guard -----------------------------------------------------------------------------------------------------------------------
def planned():
    """symbol -> cases, from the planner's own answers for every case list above (the launches go through the same ConvOp)."""
    from patchgan_amd import engine as E
    out = {}
    for (geom, opcode), forms in FWD_CASES.items():
        for bits, aligned, want_sym, slices in forms:
            out.setdefault(_launched(E.ConvOp(*geom, L.ALGO_AUTO | bits), opcode, aligned), []).append((geom, opcode, bits, aligned, slices))
    for geom in WGRAD_CASES:
        for form, bits in WGRAD_FORMS.items():
            out.setdefault(E.ConvOp(*geom, L.ALGO_AUTO | bits).describe(2)[0], []).append((geom, 2, bits, True, E.ConvOp(*geom, L.ALGO_AUTO | bits).describe(2)[1]))
    return out


ALL_TESTS = ({('dense', k) for k in FWD_CASES} | {('probe', k) for k in FWD_CASES} | {('wgrad', g, f) for g in WGRAD_CASES for f in WGRAD_FORMS} |
             {('fuzz', i) for i in range(FUZZ_CASES)})


def check_plan():
    """The case lists reach every family of the stride-1 Winograd class -- the 128-tile F(2x2,4x4) instance, 1 / 2 / 4 K slices of the
    fused F(3x3,4x4) kernel, both row forms, both LDS-DMA forms, both dy tile edges of the weight gradient in both GEMM forms and both
    output tiles.  Host-side queries only (tests/test_wino1_cpu.py runs it without a GPU as well).  Returns planned()."""
    from patchgan_amd import engine as E
    plan = planned()
    print('planned:', {k: len(v) for k, v in sorted(plan.items())})
    need = {K_F2_64, K_F2_128, K_F3, K_ROW, K_ROW_S3, K_DMA2, K_DMA3, K_W64, K_W64_S3, K_W128_S3}
    assert need <= set(plan), sorted(need - set(plan))
    assert set(plan) == need, sorted(set(plan) - need)          # ... and nothing the lists do not name
    # every case sits where its list says, tile edge and K slices included
    for (geom, opcode), forms in FWD_CASES.items():
        N, Hb, Wb, Ca, Cb, s = geom
        Ho, Wo, Ci, Co = (Hb - 1, Wb - 1, Cb, Ca) if opcode == 0 else (Hb, Wb, Ca, Cb)
        for bits, aligned, want_sym, slices in forms:
            op = E.ConvOp(*geom, L.ALGO_AUTO | bits)
            assert _launched(op, opcode, aligned) == want_sym, (geom, opcode, hex(bits))
            mo = W.fwd_tile_edge(want_sym)
            assert op.kernel_flops(opcode) == 2.0 * (mo + 3) ** 2 * N * W.tiles(Ho, mo) * W.tiles(Wo, mo) * Ca * Cb, (geom, opcode, want_sym)
            if want_sym in (K_F3, K_DMA3):      # (the DMA kernel runs unsliced only: a sliced geometry would take the fused kernel instead)
                assert W.fwd_slices(N, Ho, Wo, Ci, Co) == slices, (geom, opcode, want_sym)
            if want_sym in (K_F2_64, K_DMA2):
                assert W.tiles(N * W.tiles(Ho, 2) * W.tiles(Wo, 2), 128) * W.tiles(Co, 64) < 400
            if want_sym == K_F2_128:
                assert W.tiles(N * W.tiles(Ho, 2) * W.tiles(Wo, 2), 128) * W.tiles(Co, 64) >= 400
    assert {c[4] for c in plan[K_F3]} == {1, 2, 4}, plan[K_F3]
    assert {c[1] for c in plan[K_F3] if c[4] > 1} == {0, 1}                 # sliced in both directions
    assert any(W.tiles(c[0][3 if c[1] == 0 else 4], 64) * 64 != c[0][3 if c[1] == 0 else 4] for k in (K_F2_64, K_F3, K_ROW, K_ROW_S3) for c in plan[k])
    wg = {(WGRAD_CASES[c[0]], sym.split('<')[0]) for sym in (K_W64, K_W64_S3, K_W128_S3) for c in plan[sym]}
    assert wg == {(2, 'k_wino_wgrad_gemm'), (3, 'k_wino_wgrad_gemm'), (2, 'k_wino_wgrad_gemm_s3'), (3, 'k_wino_wgrad_gemm_s3')}, wg
    assert {WGRAD_CASES[c[0]] for c in plan[K_W128_S3]} == {2, 3}
    assert any(c[4] > 1 for sym in (K_W64, K_W64_S3, K_W128_S3) for c in plan[sym])      # more than one K slice
    for geom, r in WGRAD_CASES.items():
        N, Hb, Wb, Ca, Cb, s = geom
        assert E.ConvOp(*geom, L.ALGO_AUTO).kernel_flops(2) == 2.0 * (r + 3) ** 2 * N * W.tiles(Hb - 1, r) * W.tiles(Wb - 1, r) * Ca * Cb, geom
    assert len(_fuzz_geoms()) == FUZZ_CASES
    return plan


def test_coverage_guard():
    """A planner change that moves a case off its family fails here instead of shrinking the coverage silently; and when the whole file
    ran, every planned symbol was launched.  Prints the per-symbol table of measured figures."""
    plan = check_plan()
    # what ran is what was planned (the fuzz adds no family of its own) ...
    assert _LAUNCHED <= set(plan), sorted(_LAUNCHED - set(plan))
    print(f'{"kernel symbol":38s} runs | model max e  rms e     | kernel max e rms e     | worst ratio max  rms | dense max-norm ratio')
    for sym in sorted(_FIGURES):
        f = _FIGURES[sym]
        print(f'{sym:38s} {len(f):4d} | {max(m.max for m, k in f):.3e} {max(m.rms for m, k in f):.3e} | {max(k.max for m, k in f):.3e} '
              f'{max(k.rms for m, k in f):.3e} | {max(k.max / m.max for m, k in f):11.2f} {max(k.rms / m.rms for m, k in f):5.2f} | '
              f'{min((k.maxnorm for m, k in f if k.spread < 100), default=0):.2e} .. {max((k.maxnorm for m, k in f if k.spread < 100), default=0):.2e}')
    # ... and, when the whole file ran, every planned symbol was launched
    if _RAN >= ALL_TESTS:
        assert set(plan) <= _LAUNCHED, sorted(set(plan) - _LAUNCHED)
    else:
        print('partial run: launch coverage not asserted;', len(ALL_TESTS - _RAN), 'tests did not run')
