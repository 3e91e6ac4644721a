"""The segmentation objectives beyond the reference's three on the GPU (Trainer.loss_type = 'ce' | 'focal' | 'dice' and their sums;
segloss.hip): pg_seg_loss_reduce / pg_seg_loss_value_grad against the float64 references between guards, their bits, NaNs and a
giant-stride view, and the trainer -- one-step gradients, a three-step curve, the launch modes, off-is-off, evaluation, data
parallelism, accumulation and the run-throughs -- against SegOracleTrainer.  Needs an MI355X."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import guard_util as GU
from tests import segloss_util as U
from tests.golden_util import Golden, LOSS_KEYS

pytestmark = pytest.mark.gpu

# (terms, focal_gamma, focal_alpha) of the kernel tests
MASKS = [('ce', 2, None), ('focal', 0, None), ('focal', 2, None), ('focal', 5, None), ('focal', 0, 0.25), ('focal', 2, 0.25), ('focal', 5, 0.25),
         ('dice', 2, None), ('ce+dice', 2, None), ('focal+dice', 2, 0.25), ('ce+focal+dice', 2, 0.25)]
# (N, HW, C): one pixel; odd sizes; one slab of a four-channel pixel; 64 slabs (a sample has two slabs from HW = 2048 on:
# pg_seg_loss_slabs); N * C = 320 > 256 with two channel groups; eight channel groups
SHAPES = [(1, 1, 2), (2, 7, 3), (3, 900, 4), (1, 65536, 4), (40, 16, 8), (2, 33, 32)]
C1_SHAPE = (2, 33, 1)          # focal and dice also on one channel


def _L():
    from patchgan_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _head(terms):
    return 'softmax' if 'ce' in terms else 'sigmoid'


def _mask_id(m):
    return f'{m[0]}-g{m[1]}-a{m[2]}'


# ---------------------------------------------------------------------------------------------- A. the kernels
def _layouts(C):
    """name -> (ld, channel offset) of p and y, (ld, offset) of g.  'step': the training step's own views -- the mask channels start 3
    floats into a wider pixel (8 floats where they fit), so the base is 4-byte aligned only, and the gradient is dense.  'odd': all
    three views 2 floats into a pixel of C + 2: the 8-byte and the mixed-alignment accesses, for loads and stores."""
    wide = 8 if C <= 5 else C + 8
    return {'dense': ((C, 0), (C, 0)), 'step': ((wide, 3), (C, 0)), 'odd': ((C + 2, 2), (C + 2, 2))}


class _Views:
    """p and y in guarded views of one layout, a guarded gradient view, value word and workspace."""

    def __init__(self, p, y, layout, grad=True):
        N, HW, C = p.shape
        (ld, off), (ldg, offg) = _layouts(C)[layout]
        nchw = lambda t: t.permute(0, 2, 1).reshape(N, C, 1, HW).float()
        self.shape = (N, HW, C)
        self.pv, self.pg = GU.view_from(nchw(p), ld, off)
        self.yv, self.yg = GU.view_from(nchw(y), ld, off)
        self.gv, self.gg = GU.view(N, 1, HW, C, ldg, offg) if grad else (None, None)
        self.val = GU.flat(4)
        self.need = int(_L().load().pg_seg_loss_workspace_bytes(N, HW, C))
        self.ws = GU.flat(self.need)

    def grad(self):
        N, HW, C = self.shape
        return GU.read_nchw(self.gv).reshape(N, C, HW).permute(0, 2, 1).float().cpu().numpy().copy()

    def value(self):
        return self.val.inner(torch.float32).cpu().numpy().copy()[0]

    def slabs(self):
        N, HW, C = self.shape
        return self.ws.inner(torch.float64).cpu().numpy().copy().reshape(N, -1, C, 5)


def _launch(v, st, check=True, stream=None):
    """Both launches over the views v with the settings st; -> (value as np.float32, gradient (N, HW, C) float32 or None)."""
    L = _L()
    lib = L.load()
    N, HW, C = v.shape
    s = stream if stream is not None else _stream()
    assert lib.pg_seg_loss_reduce(v.pv.ptr(), v.pv.ld, v.yv.ptr(), v.yv.ld, N, HW, C, st.terms, st.gamma, st.alpha_arg(), v.ws.ptr(), v.need, s) == 0
    sc = st.scales(N, HW, C)
    gp, gl = (v.gv.ptr(), v.gv.ld) if v.gv is not None else (None, 0)
    assert lib.pg_seg_loss_value_grad(v.ws.ptr(), v.need, v.pv.ptr(), v.pv.ld, v.yv.ptr(), v.yv.ld, N, HW, C, st.terms, st.gamma, st.alpha_arg(),
                                      st.smooth, sc[0], sc[1], sc[2], gp, gl, v.val.ptr(), s) == 0
    torch.cuda.synchronize()
    if check:
        GU.assert_untouched(v.val, 'all', 'value')
        GU.assert_untouched(v.ws, 'all', 'workspace')
        if v.gg is not None:
            GU.assert_untouched(v.gg, 'slice', 'gradient')
    return v.value(), (v.grad() if v.gv is not None else None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _settings(terms, g, fa, N, HW):
    return U.Settings(terms, g, fa, 0.5 if HW == 7 else 1.0, alpha=200.0, bglobal=N if N % 2 else 2 * N)


def _kernel_case(terms, g, fa, shape):
    N, HW, C = shape
    p, y = U.inputs(N, HW, C, _head(terms), 1000 + N + HW + C)
    st = _settings(terms, g, fa, N, HW)
    want = U.Expect(p, y, st)
    worst = [0.0, 0.0]
    for layout in _layouts(C):
        v = _Views(p, y, layout)
        ins = GU.Inputs()
        ins.add(v.pg, 'p')
        ins.add(v.yg, 'y')
        value, grad = _launch(v, st)
        rv, rg = want.ratios(value, grad)
        print(f'pg_seg_loss {terms} g={g} alpha={fa} {shape} {layout}: value {rv:.3f}, gradient {rg:.3f} of the bound')
        worst = [max(worst[0], rv), max(worst[1], rg)]
        assert rv <= 1.0 and rg <= 1.0, (terms, g, fa, shape, layout, rv, rg)
        # value only: the same value bits, no gradient buffer to touch; the layouts agree bit for bit
        only = _Views(p, y, layout, grad=False)
        assert _bits(_launch(only, st)[0]) == _bits(value)
        if layout == 'dense':
            first = (value, grad)
        else:
            assert _bits(value) == _bits(first[0]) and np.array_equal(_bits(grad), _bits(first[1]))
        ins.check('pg_seg_loss')
    return worst


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('mask', MASKS, ids=_mask_id)
def test_kernel_against_float64(mask, shape):
    """Value and every gradient element within the derived tolerances of tests/segloss_util.py, in three layouts, between guards: pad
    channels and both sides of every buffer unchanged, the inputs unchanged.  Measured on an MI355X, worst ratio over all 216 calls
    (1 is the bound): value 0.278 (dice, (3, 900, 4)), gradient 0.311 (ce+dice, (1, 65536, 4)); the three layouts agree bit for bit."""
    _kernel_case(*mask, shape)


@pytest.mark.parametrize('mask', [m for m in MASKS if 'ce' not in m[0]], ids=_mask_id)
def test_kernel_against_float64_on_one_channel(mask):
    _kernel_case(*mask, C1_SHAPE)


def _value_from_slabs(slabs, st, shape):
    """The documented value from the workspace the first launch left: the slabs of every sum in slab order; the members' per-(n, c)
    terms added by 48 lanes, lane i taking the pairs i, i + 48, ... in index order, then a halving tree over 64 lanes; the selected
    members' products in the order ce, focal, dice in fp64; one rounding."""
    N, HW, C = shape
    S = np.zeros((N, C, 5))
    for z in range(slabs.shape[1]):
        S = S + slabs[:, z]
    S = S.reshape(N * C, 5)
    s = float(st.smooth)
    terms = {'ce': S[:, 3], 'focal': S[:, 4], 'dice': 1.0 - (2.0 * S[:, 0] + s) / (S[:, 1] + S[:, 2] + s)}
    total = 0.0
    for m, scale in zip(('ce', 'focal', 'dice'), st.scales(N, HW, C)):
        if m not in st.members():
            continue
        lanes = np.zeros(64)
        for i0 in range(0, N * C, 48):
            chunk = terms[m][i0:i0 + 48]
            lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
        off = 32
        while off:
            lanes[:off] = lanes[:off] + lanes[off:2 * off]
            off >>= 1
        total = total + scale * lanes[0]
    return np.float32(total)


@pytest.mark.parametrize('shape', [(3, 900, 4), (1, 65536, 4), (40, 16, 8)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('terms', ['ce+dice', 'focal+dice', 'ce+focal+dice'])
def test_a_sum_is_its_members_added_in_the_documented_order(terms, shape):
    """A member evaluated alone and inside a sum: the sum's gradient is fl32 of the members' gradients added in the order ce, focal,
    dice; its value is fl32 of the documented fp64 sum over the slabs the first launch wrote (and so is each member's)."""
    N, HW, C = shape
    p, y = U.inputs(N, HW, C, 'softmax', 31 + HW)
    st = _settings(terms, 2, 0.25, N, HW)
    v = _Views(p, y, 'step')
    value, grad = _launch(v, st)
    assert v.slabs().shape[1] == _L().load().pg_seg_loss_slabs(N, HW)
    assert _bits(value) == _bits(_value_from_slabs(v.slabs(), st, shape))
    acc = None
    for m in st.members():
        one = _settings(m, 2, 0.25, N, HW)
        vm = _Views(p, y, 'step')
        value_m, grad_m = _launch(vm, one)
        assert _bits(value_m) == _bits(_value_from_slabs(vm.slabs(), one, shape))
        acc = grad_m if acc is None else (acc + grad_m).astype(np.float32)
    assert np.array_equal(_bits(acc), _bits(grad))


def test_two_runs_on_two_streams_give_the_same_bits():
    N, HW, C = 1, 65536, 4
    p, y = U.inputs(N, HW, C, 'softmax', 9)
    st = _settings('ce+focal+dice', 2, 0.25, N, HW)
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        v = _Views(p, y, 'step')
        torch.cuda.synchronize()
        runs.append(_launch(v, st, stream=s.cuda_stream))
    assert _bits(runs[0][0]) == _bits(runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize('shape', [(3, 900, 4), (1, 65536, 4)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('terms', ['ce', 'focal', 'dice', 'ce+focal+dice'])
def test_a_nan_comes_out_as_specified(terms, shape):
    """A NaN in p at four positions: the value is NaN; ce and focal give a NaN gradient at those elements (whatever y holds there) and
    the clean run's bits elsewhere; dice gives a NaN gradient on the whole (n, c) plane of each and the clean run's bits on the others."""
    N, HW, C = shape
    p, y = U.inputs(N, HW, C, 'softmax', 17)
    st = _settings(terms, 2, None, N, HW)
    _, clean = _launch(_Views(p, y, 'dense'), st)
    flat = np.array([0, 63, N * HW * C // 2, N * HW * C - 1])
    bad = p.clone()
    bad.reshape(-1)[torch.from_numpy(flat)] = float('nan')
    value, grad = _launch(_Views(bad, y, 'dense'), st)
    assert np.isnan(value)
    hit = np.zeros(N * HW * C, dtype=bool)
    hit[flat] = True
    hit = hit.reshape(N, HW, C)
    if 'dice' in terms:
        hit = np.broadcast_to(hit.any(axis=1, keepdims=True), hit.shape)
    assert np.isnan(grad[hit]).all()
    assert np.isfinite(grad[~hit]).all() and np.array_equal(_bits(grad[~hit]), _bits(clean[~hit]))


def test_argument_errors_write_nothing():
    L = _L()
    lib = L.load()
    N, HW, C = 2, 4096, 4
    p, y = U.inputs(N, HW, C, 'softmax', 2)
    v = _Views(p, y, 'step')
    snaps = [v.pg.snapshot(), v.yg.snapshot()]
    ok = dict(p=v.pv.ptr(), ld_p=v.pv.ld, y=v.yv.ptr(), ld_y=v.yv.ld, N=N, HW=HW, C=C, terms=L.SEG_CE | L.SEG_DICE, gamma=2, fa=L.SEG_FOCAL_ALPHA_NONE,
              smooth=1.0, ws=v.ws.ptr(), nb=v.need, g=v.gv.ptr(), ld_g=v.gv.ld, value=v.val.ptr())

    def reduce(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_reduce(a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'], a['fa'], a['ws'], a['nb'], _stream())

    def finish(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_value_grad(a['ws'], a['nb'], a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'], a['fa'],
                                          a['smooth'], 0.1, 0.1, 0.1, a['g'], a['ld_g'], a['value'], _stream())
    for kw in (dict(p=None), dict(y=None), dict(ws=None), dict(ws=v.ws.ptr() + 4), dict(nb=v.need - 8), dict(N=0), dict(HW=0), dict(C=0), dict(ld_p=3),
               dict(ld_y=3), dict(terms=0), dict(terms=8), dict(gamma=9), dict(gamma=-1), dict(fa=0.0), dict(fa=1.0), dict(fa=float('nan'))):
        assert (reduce(**kw), finish(**kw)) == (-1, -1), kw
    for kw in (dict(value=None), dict(ld_g=3), dict(smooth=0.0), dict(smooth=float('inf')), dict(smooth=float('nan'))):
        assert finish(**kw) == -1, kw          # (settings of the second launch alone)
    torch.cuda.synchronize()
    for g, what in ((v.val, 'value'), (v.ws, 'workspace'), (v.gg, 'gradient')):
        GU.assert_untouched(g, None, what)
    GU.assert_unchanged(v.pg, snaps[0], 'p')
    GU.assert_unchanged(v.yg, snaps[1], 'y')


def test_giant_stride_views():
    """One view at a time with a pixel stride that puts its last quarter of pixels beyond a 32-bit byte offset (tier W of
    tests/bigview_util.py), the others compact: the bits of the all-compact call, and nothing written in the arena but the view."""
    from tests import bigview_util as B
    N, HW, C = 2, 12, 3
    P = N * HW
    ld = B.choose_ld('W', P, C, 4)
    need = B.region_bytes(P, ld, 4)
    assert B.quarter_start(P) * ld * 4 >= 1 << 32 and B.admissible(P, ld, C, 4)
    free = torch.cuda.mem_get_info()[0]
    if free < need + 2 * B.GIB:
        pytest.skip(f'the giant view needs a {need / B.GIB:.1f} GiB arena, torch.cuda.mem_get_info() shows {free / B.GIB:.1f} GiB free')
    L = _L()
    lib = L.load()
    p, y = U.inputs(N, HW, C, 'softmax', 4)
    st = _settings('ce+focal+dice', 2, 0.25, N, HW)
    sc = st.scales(N, HW, C)
    arena = B.Arena((need + 15) // 16 * 16, 'cuda')
    data = {'p': p.reshape(P, C).float().cuda(), 'y': y.reshape(P, C).float().cuda()}
    results = {}
    for giant in (None, 'p', 'y', 'g'):
        a, keep = {}, {}
        nbytes = 0
        for key in ('p', 'y', 'g'):
            if key == giant:
                nbytes = arena.region(P, ld, False)
                arena.fill(nbytes)
                if key in data:
                    arena.pixels(P, ld, C).copy_(data[key])
                a[key] = (arena.view(1, 1, P, C, ld).ptr(), ld)
            else:
                t = keep[key] = torch.full((P, C), float('nan'), device='cuda')
                if key in data:
                    t.copy_(data[key])
                a[key] = (t.data_ptr(), C)
        wsb = int(lib.pg_seg_loss_workspace_bytes(N, HW, C))
        ws, val = torch.empty(wsb // 8, dtype=torch.float64, device='cuda'), torch.full((1,), float('nan'), device='cuda')
        L.check(lib.pg_seg_loss_reduce(a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, st.terms, st.gamma, st.alpha_arg(), ws.data_ptr(), wsb,
                                       _stream()), 'pg_seg_loss_reduce')
        L.check(lib.pg_seg_loss_value_grad(ws.data_ptr(), wsb, a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, st.terms, st.gamma, st.alpha_arg(),
                                           st.smooth, sc[0], sc[1], sc[2], a['g'][0], a['g'][1], val.data_ptr(), _stream()), 'pg_seg_loss_value_grad')
        torch.cuda.synchronize()
        g = (arena.pixels(P, ld, C) if giant == 'g' else keep['g']).clone()
        results[giant] = (val.cpu().numpy(), g.cpu().numpy())
        assert not np.isnan(results[giant][0]).any() and not np.isnan(results[giant][1]).any()
        if giant is not None:
            found = arena.count(nbytes)
            print(f'giant {giant}: ld {ld}, last pixel at byte offset {(P - 1) * ld * 4}, {found} non-NaN elements in the arena (entitled {P * C})')
            assert found == P * C, (giant, found)
            assert _bits(results[giant][0]) == _bits(results[None][0]) and np.array_equal(_bits(results[giant][1]), _bits(results[None][1])), giant
    del arena
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- B. the trainer
SOFTMAX, SIGMOID = 'd_softmax_tversky', 'a_lrelu_tversky'          # softmax over 4 classes; sigmoid on one channel
# (fixture, loss_type, focal_gamma, focal_alpha, dice_smooth)
STEP_CASES = [(SOFTMAX, 'ce', 2, None, 1.0), (SOFTMAX, 'dice', 2, None, 1.0), (SOFTMAX, 'ce+dice', 2, None, 1.0), (SOFTMAX, 'focal', 2, None, 1.0),
              (SIGMOID, 'dice', 2, None, 1.0), (SIGMOID, 'focal+dice', 2, 0.25, 0.5)]


def _case_id(c):
    return f'{c[0][0]}-{c[1]}'


def _nets(gold, nf=None, ndf=None, g_kw=None, **dkw):
    """The fixture's networks with its weights; another width or option: torch's initialisation."""
    import patchgan_amd as pg
    c = gold.cfg
    g = pg.UNet(c['in_nc'], c['out_nc'], nf or c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'], **(g_kw or {}))
    d = pg.Discriminator(c['in_nc'] + c['out_nc'], ndf or c['ndf'], n_layers=c['n_layers'], norm=dkw.pop('norm', c['norm']), **dkw)
    if nf is None and not g_kw:
        g.load_state_dict(gold.weights('g0'))
    if ndf is None and not dkw:
        d.load_state_dict(gold.weights('d0'))
    return g.cuda(), d.cuda()


def _trainer(g, d, folder, loss_type, gamma=2, fa=None, smooth=1.0, mode=None, **attrs):
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(folder))
    t.loss_type, t.focal_gamma, t.focal_alpha, t.dice_smooth = loss_type, gamma, fa, smooth
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers(1e-3, 1e-3)
    if mode is not None:
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    g.train()
    d.train()
    return t


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _row(l):
    return [float(l[k]) for k in LOSS_KEYS]


@pytest.mark.parametrize('case', STEP_CASES, ids=_case_id)
def test_one_step_gradients_against_the_float64_oracle(tmp_path, case):
    """Every parameter's gradient of both networks after one training step against SegOracleTrainer(float64): relative L2 < 2e-2 and
    <= 8 x noise + 1e-3, noise the fp32 oracle's own distance (the metric and bound of
    test_ganloss_gpu.py::test_one_step_gradients_against_the_float64_oracle).  Measured on an MI355X: every parameter's gradient at most
    2.7e-05 in relative L2 from its float64 oracle; the worst share of its bound per case: softmax fixture ce 0.011, dice 0.026, ce+dice
    0.013, focal 0.013; sigmoid fixture dice 0.006, focal+dice 0.007."""
    name, loss_type, gamma, fa, smooth = case
    gold = Golden(name)
    x, y = gold.inputs()
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path, loss_type, gamma, fa, smooth)
    t.batch(x, y, train=True)
    t.flush()
    got = {'g_grads': {k: v.grad.detach().cpu() for k, v in g.named_parameters()}, 'd_grads': {k: v.grad.detach().cpu() for k, v in d.named_parameters()}}
    refs = {}
    for tag, dtype in (('o64', torch.float64), ('o32', torch.float32)):
        o = U.seg_oracle(gold, dtype, loss_type, gamma, fa, smooth)
        o.batch(x, y, train=True)
        refs[tag] = o.last
    worst = 0.0
    for which in ('g_grads', 'd_grads'):
        assert set(got[which]) == set(refs['o64'][which])
        for k, want in refs['o64'][which].items():
            e, noise = _l2(got[which][k], want), _l2(refs['o32'][which][k], want)
            print(f'{loss_type} {which} {k:40s} error {e:.2e} fp32-oracle noise {noise:.2e}')
            worst = max(worst, e / (8 * noise + 1e-3))
            assert e < 2e-2 and e <= 8 * noise + 1e-3, (k, e, noise)
    print(f'{name} {loss_type}: worst error {worst:.3f} of its bound')
    t.release()


# The distance of a run from SegOracleTrainer(float64) on the same run is ONE number, test_ganloss_gpu.py's _curve_dist: the largest
# relative error among the 18 loss scalars (each relative to its own value, floor 1e-6) and the parameter tensors of both networks
# after the third step (relative max-norm).  SegOracleTrainer(float32)'s own distance, computed on the CPU -- the bound is 3 x that:
CURVE_CASES = {'ce+dice': (SOFTMAX, 'ce+dice', 2, None, 1.0), 'focal': (SIGMOID, 'focal', 2, None, 1.0)}
CURVE_NOISE = {'ce+dice': 1.978e-03, 'focal': 5.323e-04}          # (the largest term is a weight tensor both times; the losses alone: 5.2e-07, 1.7e-07)


def _curve_dist(curve, want, weights, want_w):
    e_l = float((np.abs(curve - want) / np.maximum(np.abs(want), 1e-6)).max())
    e_w = max(float((weights[k].double().cpu() - w.double()).abs().max() / w.double().abs().max()) for k, w in want_w.items())
    return e_l, e_w


def _oracle_weights(o):
    return {**{'g.' + k: v.detach() for k, v in o.gw.items()}, **{'d.' + k: v.detach() for k, v in o.dw.items()}}


@pytest.mark.parametrize('key', list(CURVE_CASES))
def test_three_step_curve_against_the_float64_oracle(tmp_path, key):
    """Three training steps: the six losses of every step and the final weights of both networks.  Measured on an MI355X (distance; the
    losses alone; the bound): ce+dice 5.776e-03 (4.9e-06; 5.934e-03), focal 4.092e-04 (4.3e-07; 1.597e-03)."""
    name, loss_type, gamma, fa, smooth = CURVE_CASES[key]
    gold = Golden(name)
    x, y = gold.inputs()
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path, loss_type, gamma, fa, smooth)
    o64 = U.seg_oracle(gold, torch.float64, loss_type, gamma, fa, smooth)
    curve, want = [], []
    for s in range(3):
        l, w = t.batch(x, y, train=True), o64.batch(x, y, train=True)
        curve.append(_row(l))
        want.append([w[k] for k in LOSS_KEYS])
    t.flush()
    got_w = {**{'g.' + k: v for k, v in g.state_dict().items()}, **{'d.' + k: v for k, v in d.state_dict().items()}}
    e_l, e_w = _curve_dist(np.array(curve), np.array(want), got_w, _oracle_weights(o64))
    bound = 3 * CURVE_NOISE[key]
    print(f'{key} 3-step curve vs float64 oracle: losses {e_l:.3e}, weights {e_w:.3e}; distance {max(e_l, e_w):.3e}, bound {bound:.3e}')
    assert max(e_l, e_w) <= bound, (e_l, e_w)
    t.release()


STEPS = 6          # the captured step replays from its 4th step on (Trainer.GRAPH_WARM_STEPS = 3): three replays
_MODE_RUNS = {}


def _mode_run(tmp_path_factory, mode):
    if mode not in _MODE_RUNS:
        gold = Golden(SOFTMAX)
        g, d = _nets(gold)
        x, y = gold.inputs()
        t = _trainer(g, d, tmp_path_factory.mktemp('seg_mode'), 'ce+dice', mode=mode)
        rows, modes = [], []
        for s in range(STEPS):
            rows.append(_row(t.batch(x, y, train=True)))
            modes.append(t.launch_mode)
        t.flush()
        torch.cuda.synchronize()
        _MODE_RUNS[mode] = dict(losses=np.array(rows), modes=modes, g=g.flat.cpu().numpy().copy(), d=d.flat.cpu().numpy().copy())
        t.release()
    return _MODE_RUNS[mode]


@pytest.mark.parametrize('mode', ['eager2', 'graph'])
def test_launch_modes_are_bit_identical(tmp_path_factory, mode):
    one, other = _mode_run(tmp_path_factory, 'eager1'), _mode_run(tmp_path_factory, mode)
    assert other['modes'][3:] == [mode] * (STEPS - 3) and one['modes'] == ['eager1'] * STEPS, (one['modes'], other['modes'])
    assert np.array_equal(one['losses'], other['losses']), one['losses'] - other['losses']
    assert np.array_equal(one['g'], other['g']) and np.array_equal(one['d'], other['d'])
    assert np.isfinite(one['losses']).all()


def test_a_changed_gamma_is_another_kind_of_step(tmp_path):
    """focal_gamma is a launch argument: a captured step holds the value it was captured with.  After six steps with gamma = 2 (three of
    them replays) the attribute changes to 5: the next step is another kind -- launched eagerly again, captured again after its warm
    steps -- and its losses are, bit for bit, those of a trainer that never captured anything and changed gamma at the same step."""
    gold = Golden(SIGMOID)
    x, y = gold.inputs()
    runs = {}
    for mode in ('graph', 'eager1'):
        g, d = _nets(gold)
        t = _trainer(g, d, tmp_path / mode, 'focal+dice', 2, 0.25, 1.0, mode=mode)
        rows, modes = [], []
        for s in range(2 * STEPS):
            if s == STEPS:
                t.focal_gamma = 5
            rows.append(_row(t.batch(x, y, train=True)))
            modes.append(t.launch_mode)
        t.flush()
        torch.cuda.synchronize()
        runs[mode] = (np.array(rows), modes, g.flat.cpu().numpy().copy())
        t.release()
    rows, modes, gw = runs['graph']
    assert modes[3:STEPS] == ['graph'] * (STEPS - 3) and modes[STEPS] != 'graph' and modes[STEPS + 3:] == ['graph'] * (STEPS - 3), modes
    assert np.array_equal(rows, runs['eager1'][0]) and np.array_equal(gw, runs['eager1'][2])
    # ... and gamma does change the objective: with 2 kept throughout, step 7 reports another loss
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path / 'kept', 'focal+dice', 2, 0.25, 1.0, mode='eager1')
    kept = np.array([_row(t.batch(x, y, train=True)) for _ in range(STEPS + 1)])
    t.release()
    assert np.array_equal(kept[:STEPS], rows[:STEPS]) and kept[STEPS, 0] != rows[STEPS, 0]


class _Recorder:
    """Stands in for the loaded library: records every entry point reached with its arguments that are not addresses, calls through."""

    def __init__(self, lib, L):
        self._lib, self._L, self.calls = lib, L, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('pg_'):
            return fn
        kinds = self._L.SIGNATURES[name][1]

        def call(*args):
            self.calls.append((name, tuple(a for a, k in zip(args, kinds) if k in (self._L._i, self._L._l, self._L._f, self._L._d))))
            if name == 'pg_seg_loss_value_grad':
                self.calls[-1] += ('g' if args[16] else 'no g',)
            return fn(*args)
        return call

    @property
    def names(self):
        return [c[0] for c in self.calls]


def _recorded(tmp_path, monkeypatch, tag, fixture=SIGMOID, nsteps=3, train=True, **attrs):
    L = _L()
    gold = Golden(fixture)
    x, y = gold.inputs()
    g, d = _nets(gold)
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(tmp_path / tag))
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers(1e-3, 1e-3)
    g.train()
    d.train()
    rec = _Recorder(L.load(), L)
    monkeypatch.setattr(L, '_lib', rec)
    rows = [_row(l) for l in (t.batch(x, y, train=train) for _ in range(nsteps))]
    t.flush()
    torch.cuda.synchronize()
    monkeypatch.undo()
    out = (np.array(rows), g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy(), rec)
    t.release()
    return out


SEG_ENTRY = ('pg_seg_loss_workspace_bytes', 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')
REF_TERM = ('pg_loss_reduce_doubles', 'pg_loss_reduce_parts', 'pg_loss_value_grad')


def test_off_is_off_and_the_launch_counts(tmp_path, monkeypatch):
    """A trainer whose attributes were never set and one with focal_gamma = 5, dice_smooth = 0.5 set while loss_type = 'tversky': the same
    library calls with the same arguments, the same bits, never a new entry point.  With 'dice': exactly one pg_seg_loss_reduce and one
    pg_seg_loss_value_grad per step, pg_loss_reduce_parts three times instead of four (the three BCE terms), everything else the off
    trainer's sequence."""
    never = _recorded(tmp_path, monkeypatch, 'never')
    inert = _recorded(tmp_path, monkeypatch, 'inert', focal_gamma=5, focal_alpha=0.25, dice_smooth=0.5, loss_type='tversky')
    dice = _recorded(tmp_path, monkeypatch, 'dice', loss_type='dice')
    for a, b in zip(never[:3], inert[:3]):
        assert np.array_equal(a, b)
    assert never[3].calls == inert[3].calls and len(never[3].calls) > 100
    assert not any('seg_loss' in n for n in never[3].names)
    assert all(never[3].names.count(n) == 4 * 3 for n in REF_TERM)
    on = dice[3].names
    assert all(on.count(n) == 3 for n in SEG_ENTRY) and all(on.count(n) == 3 * 3 for n in REF_TERM)
    assert all(c[-1] == 'g' for c in dice[3].calls if c[0] == 'pg_seg_loss_value_grad')
    other = lambda rec: [c for c in rec.calls if c[0] not in SEG_ENTRY + REF_TERM]
    assert other(dice[3]) == other(never[3])
    # the two launches sit where the reference pair sat: the first in front of the discriminator's forward pass, the second behind it
    seq = lambda rec, a, b: [n for n in rec.names if n in (a, b) or n.startswith('pg_conv4x4')]
    place = lambda s, a, b: [i for i, n in enumerate(s) if n in (a, b)][:2]
    s_off, s_on = seq(never[3], 'pg_loss_reduce_parts', 'pg_loss_value_grad'), seq(dice[3], 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')
    assert place(s_off, 'pg_loss_reduce_parts', 'pg_loss_value_grad') == place(s_on, 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')
    assert place(s_on, 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')[1] - place(s_on, 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')[0] > 1
    assert not np.array_equal(dice[0], never[0])


@pytest.mark.parametrize('key', list(CURVE_CASES))
def test_evaluation_values_and_no_update(tmp_path, monkeypatch, key):
    """batch(train=False) and evaluate(): the values against the float64 oracle within the curve bound, pg_seg_loss_value_grad without a
    gradient, no Adam launch, no weight of either network changed; metrics = True adds its one launch and reads back.  Measured on an
    MI355X: every value within 8.6e-08 (ce+dice) and 7.7e-08 (focal) of the oracle's, evaluate()'s seg_loss within 5.5e-08 and 4.5e-08."""
    name, loss_type, gamma, fa, smooth = CURVE_CASES[key]
    gold = Golden(name)
    x, y = gold.inputs()
    g, d = _nets(gold)
    g0, d0 = g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy()
    rows, g1, d1, rec = _recorded(tmp_path, monkeypatch, 'eval', name, nsteps=1, train=False, loss_type=loss_type, focal_gamma=gamma,
                                  focal_alpha=fa, dice_smooth=smooth, metrics=True)
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert rec.names.count('pg_seg_loss_reduce') == 1 and rec.names.count('pg_seg_confusion') == 1
    assert [c[-1] for c in rec.calls if c[0] == 'pg_seg_loss_value_grad'] == ['no g'] and not any(n.startswith('pg_adam') for n in rec.names)
    o = U.seg_oracle(gold, torch.float64, loss_type, gamma, fa, smooth)
    want = o.batch(x, y, train=False)
    bound = 3 * CURVE_NOISE[key]
    for i, k in enumerate(LOSS_KEYS):
        e = abs(rows[0, i] - want[k]) / max(abs(want[k]), 1e-6)
        print(f'{key} evaluation step: {k} {rows[0, i]:.8f} oracle {want[k]:.8f} rel {e:.2e}')
        assert e <= bound, (k, e)
    t = _trainer(g, d, tmp_path / 'evaluate', loss_type, gamma, fa, smooth, metrics=True)
    out = t.evaluate([(x, y), (x, y)])
    e = abs(out['seg_loss'] - o.last['seg']) / abs(o.last['seg'])
    print(f'{key} evaluate(): seg_loss {out["seg_loss"]:.8f} oracle {o.last["seg"]:.8f} rel {e:.2e}')
    assert e <= bound and 'miou' in out and np.array_equal(g.flat.cpu().numpy(), g0)
    t.batch(x, y, train=False)
    assert 'miou' in t.read_metrics()
    t.release()


# ---------------------------------------------------------------------------------------------- C. batch consistency
DP_LOSS = ('focal+dice', 2, 0.25, 1.0)


def _dp_worker(rank, world, port, q, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    gold = Golden(SIGMOID)
    g, d = _nets(gold)
    x, y = gold.inputs()
    t = _trainer(g, d, tempfile.mkdtemp(), *DP_LOSS)
    xs, ys = shard_batch(x, y, rank, world)
    curve = [_row(t.batch(xs, ys, train=True)) for _ in range(nsteps)]
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, np.array(curve), g.flat.cpu().numpy(), d.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_against_the_single_process(tmp_path):
    """focal+dice on two ranks (gloo, both on the one GPU), each with half of the batch, against the single process on the whole batch:
    the comparison and bound of tests/test_dp_gpu.py for the default step.  Measured on an MI355X: losses within 9.8e-08."""
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    nsteps = 3
    gold = Golden(SIGMOID)
    g, d = _nets(gold)
    x, y = gold.inputs()
    assert x.shape[0] == 2
    t = _trainer(g, d, tmp_path, *DP_LOSS)
    single = np.array([_row(l) for l in (t.batch(x, y, train=True) for _ in range(nsteps))])
    t.release()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, nsteps)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, g0, d0), (_, c1, g1, d1) = res
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert np.allclose(c0, c1, rtol=1e-6)
    err = np.abs(c0 - single) / np.maximum(np.abs(single), 1e-6)
    print('focal+dice dp2 vs single process: max rel err per step', err.max(axis=1))
    assert err.max() < 1e-4, err


def test_window_of_two_halves_is_the_batch_of_four(tmp_path):
    """accumulate = 2 over the two halves of a batch of four against a trainer without the feature on the whole batch, for focal+dice:
    the comparison tests/test_accum_gpu.py makes for MAE -- relative L2 < 1e-5, norm ratio within 1e-5 of 1, losses to 1e-6.  Measured on an
    MI355X: relative L2 7.7e-08 (G) and 8.2e-07 (D), norm ratio 1.0000000, losses within 4.9e-08."""
    gold = Golden(SIGMOID)
    c = gold.cfg
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(4, c['in_nc'], c['size'], c['size'], generator=gen)
    y = (torch.rand(4, c['out_nc'], c['size'], c['size'], generator=gen) > 0.7).float()

    def grads(t):
        t.flush()
        torch.cuda.synchronize()
        return t.generator.grad_flat.cpu().numpy().copy(), t.discriminator.grad_flat.cpu().numpy().copy()
    big = _trainer(*_nets(gold), tmp_path / 'big', *DP_LOSS)
    want_loss = np.array(_row(big.batch(x, y, train=True)))
    want = grads(big)
    t = _trainer(*_nets(gold), tmp_path / 'acc', *DP_LOSS, accumulate=2)
    rows = np.array([_row(t.batch(x[:2], y[:2], train=True)), _row(t.batch(x[2:], y[2:], train=True))])
    got = grads(t)
    for name, a, b in (('G', got[0], want[0]), ('D', got[1], want[1])):
        a, b = a.astype(np.float64), b.astype(np.float64)
        rel, ratio = np.linalg.norm(a - b) / np.linalg.norm(b), np.linalg.norm(a) / np.linalg.norm(b)
        print(f'window of two halves vs the batch of four, {name} gradient: relative L2 {rel:.2e}, norm ratio {ratio:.7f}')
        assert rel < 1e-5 and abs(ratio - 1) < 1e-5, (name, rel, ratio)
    err = np.abs(rows.mean(axis=0) - want_loss) / np.maximum(np.abs(want_loss), 1e-6)
    print(f'mean of the two calls losses vs the large batch: relative error {err}')
    assert err.max() < 1e-6, err
    assert (t._t_g, t._t_d) == (1, 1) == (big._t_g, big._t_d)
    big.release()
    t.release()


# ---------------------------------------------------------------------------------------------- D. run-throughs
def _smoke(t, x, y, nsteps=2):
    rows = [_row(l) for l in (t.batch(x, y, train=True) for _ in range(nsteps))]
    t.flush()
    torch.cuda.synchronize()
    assert np.isfinite(rows).all(), rows
    return np.array(rows)


def test_every_option_together_on_bf16_networks(tmp_path):
    """ce+focal+dice with bf16 networks (InstanceNorm: bf16 precision is not implemented for BatchNorm networks, which have the next test),
    hinge on a spectrally normalised logit discriminator, diffaug, clipping and the weight average."""
    torch.manual_seed(3)
    gold = Golden(SOFTMAX)
    g, d = _nets(gold, nf=16, ndf=32, spectral_norm=True, final_act='none')
    g.set_precision('bf16')
    d.set_precision('bf16')
    x, y = gold.inputs()
    t = _trainer(g, d, tmp_path, 'ce+focal+dice', 2, 0.25, 1.0, gan_mode='hinge', ema_decay=0.99, diffaug='flip,translation,cutout', diffaug_seed=8,
                 clip_grad_norm=1.0, two_streams=True)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all() and torch.isfinite(t.ema_generator.flat).all()
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['gen']['skipped'] == 0 and stats['disc']['skipped'] == 0
    t.release()


def test_every_option_together_on_batchnorm_networks(tmp_path):
    """The same options on fp32 nn.BatchNorm2d networks (bf16 precision is not implemented for them): ce+dice, hinge on a spectrally
    normalised logit discriminator, diffaug, clipping and the weight average."""
    from torch import nn
    torch.manual_seed(3)
    gold = Golden(SOFTMAX)
    g, d = _nets(gold, g_kw=dict(norm_layer=nn.BatchNorm2d), norm=True, norm_layer=nn.BatchNorm2d, spectral_norm=True, final_act='none')
    x, y = gold.inputs()
    x, y = torch.cat((x, x.flip(3))), torch.cat((y, y.flip(3)))          # (batch statistics want more than one sample)
    t = _trainer(g, d, tmp_path, 'ce+dice', gan_mode='hinge', ema_decay=0.99, diffaug='flip,translation,cutout', diffaug_seed=8, clip_grad_norm=1.0,
                 two_streams=True)
    _smoke(t, x, y)
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all() and torch.isfinite(t.ema_generator.flat).all()
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['gen']['skipped'] == 0 and stats['disc']['skipped'] == 0
    t.release()


def test_a_nan_in_the_target_skips_the_step(tmp_path):
    """A NaN in y reaches the value and the generator's gradient through every objective; with clip_grad_norm set the generator's
    update is skipped and its weights keep their bits."""
    gold = Golden(SOFTMAX)
    x, y = gold.inputs()
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path, 'ce+dice', clip_grad_norm=10.0)
    t.batch(x, y, train=True)
    t.flush()
    before = g.flat.cpu().numpy().copy()
    bad = y.clone()
    bad[0, 1, 100, 100] = float('nan')
    l = t.batch(x, bad, train=True)
    t.flush()
    torch.cuda.synchronize()
    assert np.isnan(l['gen'])
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['gen']['skipped'] == 1
    assert np.array_equal(g.flat.cpu().numpy(), before)
    t.release()
