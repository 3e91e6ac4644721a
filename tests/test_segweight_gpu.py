"""Per-class weights of the segmentation objectives on the GPU (Trainer.class_weights; segloss.hip): pg_seg_loss_value_grad_w against
the weighted float64 references between guards, its bits (all-ones weights = the unweighted entry point, zero weights, two streams,
NaNs, a giant-stride view), pg_seg_label_count against NumPy, and the trainer -- one-step gradients against the weighted float64
oracle, the launch modes, off-is-off, evaluation, the estimate and its file, two ranks, and a run-through.  Needs an MI355X."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from tests import guard_util as GU
from tests import segloss_util as U
from tests import segweight_util as WU
from tests.golden_util import Golden
from tests.test_segloss_gpu import SIGMOID, SOFTMAX, STEPS, _bits, _head, _L, _l2, _launch, _nets, _recorded, _row, _settings, _stream, _trainer, _Views

pytestmark = pytest.mark.gpu

# (terms, focal_gamma, focal_alpha)
MASKS = [('ce', 2, None), ('focal', 0, None), ('focal', 2, None), ('focal', 0, 0.25), ('focal', 2, 0.25), ('dice', 2, None), ('ce+focal+dice', 2, 0.25)]
# (N, HW, C): one pixel with a partial channel group; odd sizes; one group; N * C = 320 pairs in two groups; eight groups; 64 slabs
SHAPES = [(1, 1, 2), (2, 7, 3), (3, 900, 4), (40, 16, 8), (2, 33, 32), (1, 65536, 4)]
LAYOUTS = ('dense', 'step')          # 'step': the mask slice starts 3 floats into a pixel of 8 (C <= 5) or C + 8 floats
W4 = [0.1, 37.5, 0.0, 1.0]


def _mask_id(m):
    return f'{m[0]}-g{m[1]}-a{m[2]}'


def _shape_id(s):
    return 'x'.join(map(str, s))


# ---------------------------------------------------------------------------------------------- A. pg_seg_loss_value_grad_w
def _launch_w(v, st, w, check=True, stream=None):
    """pg_seg_loss_reduce, then pg_seg_loss_value_grad_w with the weights w in a guarded device buffer, over the views v;
    -> (value as np.float32, gradient (N, HW, C) float32 or None)."""
    lib = _L().load()
    N, HW, C = v.shape
    s = stream if stream is not None else _stream()
    cw = GU.flat_from(torch.tensor(w, dtype=torch.float32))
    snap = cw.snapshot()
    assert lib.pg_seg_loss_reduce(v.pv.ptr(), v.pv.ld, v.yv.ptr(), v.yv.ld, N, HW, C, st.terms, st.gamma, st.alpha_arg(), v.ws.ptr(), v.need, s) == 0
    sc = st.scales(N, HW, C)
    gp, gl = (v.gv.ptr(), v.gv.ld) if v.gv is not None else (None, 0)
    assert lib.pg_seg_loss_value_grad_w(v.ws.ptr(), v.need, v.pv.ptr(), v.pv.ld, v.yv.ptr(), v.yv.ld, N, HW, C, st.terms, st.gamma, st.alpha_arg(),
                                        st.smooth, sc[0], sc[1], sc[2], cw.ptr(), gp, gl, v.val.ptr(), s) == 0
    torch.cuda.synchronize()
    if check:
        GU.assert_untouched(v.val, 'all', 'value')
        GU.assert_untouched(v.ws, 'all', 'workspace')
        if v.gg is not None:
            GU.assert_untouched(v.gg, 'slice', 'gradient')
        GU.assert_unchanged(cw, snap, 'weights')
    return v.value(), (v.grad() if v.gv is not None else None)


@pytest.mark.parametrize('shape', SHAPES, ids=_shape_id)
@pytest.mark.parametrize('mask', MASKS, ids=_mask_id)
def test_weighted_kernel_against_float64(mask, shape):
    """Value and every gradient element within the tolerances of tests/segweight_util.py (segloss_util's with scale -> scale * w_c),
    for distinct weights with a 0, a 0.1 and a 37.5 among them, on the dense views and on the step's own (the mask slice 3 floats into
    a wider pixel), between guards: the workspace as the reduction left it, pad channels, both sides of every buffer, the inputs and
    the weights unchanged; a zero-weight channel's gradient exactly +-0; the value-only call and the two layouts agree bit for bit.
    Measured on an MI355X, worst ratio over all 84 calls (1 is the bound): value 0.209 (ce, (3, 900, 4)), gradient 0.351 (ce, (40, 16, 8))."""
    terms, g, fa = mask
    N, HW, C = shape
    p, y = U.inputs(N, HW, C, _head(terms), 1000 + N + HW + C)
    st = _settings(terms, g, fa, N, HW)
    w = WU.weights_for(C)
    want = WU.Expect(p, y, st, w)
    first = None
    for layout in LAYOUTS:
        v = _Views(p, y, layout)
        ins = GU.Inputs()
        ins.add(v.pg, 'p')
        ins.add(v.yg, 'y')
        value, grad = _launch_w(v, st, w)
        rv, rg = want.ratios(value, grad)
        print(f'pg_seg_loss_value_grad_w {terms} g={g} alpha={fa} {shape} {layout}: value {rv:.3f}, gradient {rg:.3f} of the bound')
        assert rv <= 1.0 and rg <= 1.0, (terms, g, fa, shape, layout, rv, rg)
        zero = [c for c in range(C) if w[c] == 0.0]
        assert np.all(grad[..., zero] == 0.0)
        only = _Views(p, y, layout, grad=False)
        assert _bits(_launch_w(only, st, w)[0]) == _bits(value)
        if first is None:
            first = (value, grad)
        else:
            assert _bits(value) == _bits(first[0]) and np.array_equal(_bits(grad), _bits(first[1]))
        ins.check('pg_seg_loss_value_grad_w')


@pytest.mark.parametrize('shape', [(3, 900, 4), (2, 33, 32)], ids=_shape_id)
def test_all_ones_weights_give_the_unweighted_bits(shape):
    N, HW, C = shape
    p, y = U.inputs(N, HW, C, 'softmax', 21 + HW)
    st = _settings('ce+focal+dice', 2, 0.25, N, HW)
    for layout in LAYOUTS:
        value, grad = _launch(_Views(p, y, layout), st)
        value_w, grad_w = _launch_w(_Views(p, y, layout), st, [1.0] * C)
        assert _bits(value) == _bits(value_w) and np.array_equal(_bits(grad), _bits(grad_w)), layout
        assert _bits(_launch_w(_Views(p, y, layout, grad=False), st, [1.0] * C)[0]) == _bits(value)


@pytest.mark.parametrize('terms', ['ce', 'focal', 'dice', 'ce+focal+dice'])
def test_a_zero_weight_channel_gets_a_zero_gradient(terms):
    """... exactly +-0 at every element, planted p of 0, 1 and a denormal included, and the other channels keep the bits they have when
    the zero is a one (a weight acts on its own channel only); all but one weight zero: the value is that channel's alone."""
    N, HW, C = 3, 900, 4
    p, y = U.inputs(N, HW, C, _head(terms), 5)
    st = _settings(terms, 2, 0.25, N, HW)
    _, grad = _launch_w(_Views(p, y, 'step'), st, W4)
    assert np.all(grad[..., 2] == 0.0) and all(np.any(grad[..., c] != 0.0) for c in (0, 1, 3))
    _, other = _launch_w(_Views(p, y, 'step'), st, [0.1, 37.5, 1.0, 1.0])
    assert np.array_equal(_bits(grad[..., [0, 1, 3]]), _bits(other[..., [0, 1, 3]])) and np.any(other[..., 2] != 0.0)
    value, grad = _launch_w(_Views(p, y, 'step'), st, [0.0, 37.5, 0.0, 0.0])
    assert np.all(grad[..., [0, 2, 3]] == 0.0)
    rv, rg = WU.Expect(p, y, st, [0.0, 37.5, 0.0, 0.0]).ratios(value, grad)
    assert rv <= 1.0 and rg <= 1.0


def test_two_runs_on_two_streams_give_the_same_bits():
    N, HW, C = 1, 65536, 4
    p, y = U.inputs(N, HW, C, 'softmax', 9)
    st = _settings('ce+focal+dice', 2, 0.25, N, HW)
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        v = _Views(p, y, 'step')
        torch.cuda.synchronize()
        runs.append(_launch_w(v, st, W4, stream=s.cuda_stream))
    assert _bits(runs[0][0]) == _bits(runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize('terms', ['ce', 'focal', 'dice', 'ce+focal+dice'])
def test_a_nan_comes_out_as_specified_whatever_the_weight(terms):
    """A NaN in p in each of the four channels (weights 0.1, 37.5, 0 and 1), a sample apart for two of them: the value is NaN; ce and
    focal give a NaN gradient at those elements and the clean run's bits elsewhere; dice gives a NaN gradient on the whole (n, c) plane
    of each -- the zero-weight channel's too -- and the clean run's bits on the others."""
    N, HW, C = 3, 900, 4
    p, y = U.inputs(N, HW, C, 'softmax', 17)
    st = _settings(terms, 2, None, N, HW)
    _, clean = _launch_w(_Views(p, y, 'dense'), st, W4)
    where = [(0, 5, 2), (0, 77, 0), (1, 400, 1), (2, 899, 2), (2, 31, 3)]
    for only in (where, [(1, 13, 2)]):          # (... and a NaN under the zero weight alone)
        bad = p.clone()
        hit = np.zeros((N, HW, C), dtype=bool)
        for n, i, c in only:
            bad[n, i, c] = float('nan')
            hit[n, i, c] = True
        value, grad = _launch_w(_Views(bad, y, 'dense'), st, W4)
        assert np.isnan(value)
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
    cw = GU.flat_from(torch.tensor(W4, dtype=torch.float32))
    cnt = GU.flat((C + 2) * 8)
    snaps = [v.pg.snapshot(), v.yg.snapshot(), cw.snapshot()]
    ok = dict(p=v.pv.ptr(), ld_p=v.pv.ld, y=v.yv.ptr(), ld_y=v.yv.ld, N=N, HW=HW, C=C, terms=L.SEG_CE | L.SEG_DICE, gamma=2, fa=L.SEG_FOCAL_ALPHA_NONE,
              smooth=1.0, ws=v.ws.ptr(), nb=v.need, g=v.gv.ptr(), ld_g=v.gv.ld, value=v.val.ptr(), cw=cw.ptr(), counts=cnt.ptr())

    def finish(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_loss_value_grad_w(a['ws'], a['nb'], a['p'], a['ld_p'], a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['terms'], a['gamma'], a['fa'],
                                            a['smooth'], 0.1, 0.1, 0.1, a['cw'], a['g'], a['ld_g'], a['value'], _stream())

    def count(**kw):
        a = dict(ok, **kw)
        return lib.pg_seg_label_count(a['y'], a['ld_y'], a['N'], a['HW'], a['C'], a['counts'], _stream())
    for kw in (dict(cw=None), dict(p=None), dict(y=None), dict(value=None), dict(ws=None), dict(ws=v.ws.ptr() + 4), dict(nb=v.need - 8), dict(N=0), dict(HW=0),
               dict(C=0), dict(ld_p=3), dict(ld_y=3), dict(ld_g=3), dict(terms=0), dict(terms=8), dict(gamma=9), dict(gamma=-1), dict(fa=0.0), dict(fa=1.0),
               dict(fa=float('nan')), dict(smooth=0.0), dict(smooth=float('inf')), dict(smooth=float('nan'))):
        assert finish(**kw) == -1, kw
    for kw in (dict(y=None), dict(counts=None), dict(N=0), dict(HW=0), dict(C=0), dict(ld_y=3)):
        assert count(**kw) == -1, kw
    torch.cuda.synchronize()
    for g, what in ((v.val, 'value'), (v.ws, 'workspace'), (v.gg, 'gradient'), (cnt, 'counts')):
        GU.assert_untouched(g, None, what)
    GU.assert_unchanged(v.pg, snaps[0], 'p')
    GU.assert_unchanged(v.yg, snaps[1], 'y')
    GU.assert_unchanged(cw, snaps[2], 'weights')


def _giant(N, HW, C):
    from tests import bigview_util as B
    P = N * HW
    ld = B.choose_ld('W', P, C, 4)
    need = B.region_bytes(P, ld, 4)
    assert B.quarter_start(P) * ld * 4 >= 1 << 32 and B.admissible(P, ld, C, 4)
    free = torch.cuda.mem_get_info()[0]
    if free < need + 2 * B.GIB:
        pytest.skip(f'the giant view needs a {need / B.GIB:.1f} GiB arena, torch.cuda.mem_get_info() shows {free / B.GIB:.1f} GiB free')
    return B, P, ld, B.Arena((need + 15) // 16 * 16, 'cuda')


def test_giant_stride_views():
    """One view at a time with a pixel stride that puts its last quarter of pixels beyond a 32-bit byte offset (tier W of
    tests/bigview_util.py), the others compact: pg_seg_loss_value_grad_w gives the bits of the all-compact call and writes nothing in
    the arena but the view; pg_seg_label_count gives the compact target's counts and writes nothing in the arena at all."""
    N, HW, C = 2, 12, 3
    B, P, ld, arena = _giant(N, HW, C)
    L = _L()
    lib = L.load()
    p, y = U.inputs(N, HW, C, 'softmax', 4)
    st = _settings('ce+focal+dice', 2, 0.25, N, HW)
    sc = st.scales(N, HW, C)
    cw = torch.tensor(WU.weights_for(C), dtype=torch.float32, device='cuda')
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
        counts = torch.zeros(C + 2, dtype=torch.int64, device='cuda')
        L.check(lib.pg_seg_loss_reduce(a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, st.terms, st.gamma, st.alpha_arg(), ws.data_ptr(), wsb,
                                       _stream()), 'pg_seg_loss_reduce')
        L.check(lib.pg_seg_loss_value_grad_w(ws.data_ptr(), wsb, a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, st.terms, st.gamma, st.alpha_arg(),
                                             st.smooth, sc[0], sc[1], sc[2], cw.data_ptr(), a['g'][0], a['g'][1], val.data_ptr(), _stream()),
                'pg_seg_loss_value_grad_w')
        L.check(lib.pg_seg_label_count(a['y'][0], a['y'][1], N, HW, C, counts.data_ptr(), _stream()), 'pg_seg_label_count')
        torch.cuda.synchronize()
        g = (arena.pixels(P, ld, C) if giant == 'g' else keep['g']).clone()
        results[giant] = (val.cpu().numpy(), g.cpu().numpy(), counts.cpu().numpy())
        assert not np.isnan(results[giant][0]).any() and not np.isnan(results[giant][1]).any()
        assert np.array_equal(results[giant][2], WU.label_counts(y.numpy()))
        if giant is not None:
            found = arena.count(nbytes)
            print(f'giant {giant}: ld {ld}, last pixel at byte offset {(P - 1) * ld * 4}, {found} non-NaN elements in the arena (entitled {P * C})')
            assert found == P * C, (giant, found)
            assert _bits(results[giant][0]) == _bits(results[None][0]) and np.array_equal(_bits(results[giant][1]), _bits(results[None][1])), giant
    del arena
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- B. pg_seg_label_count
COUNT_SHAPES = SHAPES + [(1, 1, 1), (3, 77, 40), (2, 1500, 5)]


def _count(y, ld=None, off=0, calls=1):
    """pg_seg_label_count `calls` times over the target y (N, HW, C) in a guarded view of pixel stride ld, channel offset off, into a
    guarded, zeroed table -> the C + 2 words."""
    N, HW, C = y.shape
    lib = _L().load()
    yv, yg = GU.view_from(y.permute(0, 2, 1).reshape(N, C, 1, HW).float(), ld or C, off)
    snap = yg.snapshot()
    cnt = GU.flat((C + 2) * 8)
    cnt.inner(torch.int64).zero_()
    for _ in range(calls):
        assert lib.pg_seg_label_count(yv.ptr(), yv.ld, N, HW, C, cnt.ptr(), _stream()) == 0
    torch.cuda.synchronize()
    GU.assert_untouched(cnt, 'all', 'counts')
    GU.assert_unchanged(yg, snap, 'y')
    return cnt.inner(torch.int64).cpu().numpy().copy()


@pytest.mark.parametrize('shape', COUNT_SHAPES, ids=_shape_id)
def test_label_count_equals_numpys(shape):
    """One-hot, unlabelled, soft and multi-hot pixels, values exactly 0.5 and one ulp below it, NaNs: NumPy's counts exactly, on the
    dense target, 3 floats into a wider pixel (4-byte aligned only) and 2 floats into a pixel of C + 2; two calls add up; the table
    and nothing else is written."""
    N, HW, C = shape
    y = WU.count_target(N, HW, C, 300 + N + HW + C)
    want = WU.label_counts(y.numpy())
    assert want[-1] == N * HW and (N * HW < 100 or (want[C] > 0 and want[:C].sum() > 0))
    for ld, off in ((C, 0), (8 if C <= 5 else C + 8, 3), (C + 2, 2)):
        got = _count(y, ld, off)
        assert np.array_equal(got, want), (shape, ld, off, got, want)
    assert np.array_equal(_count(y, C + 2, 2, calls=2), 2 * want)


def test_label_count_of_a_one_hot_target_is_its_class_histogram():
    N, HW, C = 4, 4099, 4
    gen = torch.Generator().manual_seed(3)
    labels = torch.multinomial(torch.tensor([0.9, 0.07, 0.0, 0.03]), N * HW, replacement=True, generator=gen).reshape(N, HW)
    y = torch.nn.functional.one_hot(labels, C).float()
    got = _count(y)
    assert got[:C].tolist() == np.bincount(labels.reshape(-1).numpy(), minlength=C).tolist() and got[C] == 0 and got[C + 1] == N * HW and got[2] == 0


# ---------------------------------------------------------------------------------------------- C. the trainer
def _wide_sigmoid(gold, C=3):
    """The sigmoid fixture's configuration with C output channels (torch's initialisation under a fixed seed): the networks on the GPU,
    their state dicts for the oracle, and a batch."""
    import patchgan_amd as pg
    c = gold.cfg
    torch.manual_seed(11)
    g = pg.UNet(c['in_nc'], C, c['nf'], use_dropout=False, activation=c['activation'], final_act=c['final_act'])
    d = pg.Discriminator(c['in_nc'] + C, c['ndf'], n_layers=c['n_layers'], norm=c['norm'])
    sd = tuple({k: v.detach().clone() for k, v in net.state_dict().items()} for net in (g, d))
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(c['B'], c['in_nc'], c['size'], c['size'], generator=gen)
    y = (torch.rand(c['B'], C, c['size'], c['size'], generator=gen) > 0.7).float()
    return g.cuda(), d.cuda(), sd, x, y


# (fixture, loss_type, focal_gamma, focal_alpha, dice_smooth, class weights)
STEP_CASES = [(SOFTMAX, 'ce+dice', 2, None, 1.0, W4), (SIGMOID, 'focal+dice', 2, 0.25, 0.5, [0.1, 37.5, 1.0])]


def _setup(case):
    name, loss_type, gamma, fa, smooth, w = case
    gold = Golden(name)
    if name == SOFTMAX:
        g, d = _nets(gold)
        x, y = gold.inputs()
        sd = None
    else:
        g, d, sd, x, y = _wide_sigmoid(gold, len(w))
    return gold, g, d, sd, x, y


@pytest.mark.parametrize('case', STEP_CASES, ids=lambda c: f'{c[0][0]}-{c[1]}')
def test_one_step_gradients_against_the_float64_oracle(tmp_path, case):
    """Every parameter's gradient of both networks after one weighted training step against WeightedSegOracleTrainer(float64), which
    passes class_weights to the torch ops of patchgan_amd.losses: relative L2 < 2e-2 and <= 8 x noise + 1e-3, noise the fp32 oracle's
    own distance (the metric and bound of test_segloss_gpu.py::test_one_step_gradients_against_the_float64_oracle).  On the softmax
    fixture with ce+dice and on the sigmoid fixture's configuration at three output channels with focal+dice.  Measured on an MI355X,
    the worst share of its bound: softmax fixture ce+dice 0.025, sigmoid configuration focal+dice 0.003."""
    name, loss_type, gamma, fa, smooth, w = case
    gold, g, d, sd, x, y = _setup(case)
    t = _trainer(g, d, tmp_path, loss_type, gamma, fa, smooth, class_weights=w)
    t.batch(x, y, train=True)
    t.flush()
    got = {'g_grads': {k: v.grad.detach().cpu() for k, v in g.named_parameters()}, 'd_grads': {k: v.grad.detach().cpu() for k, v in d.named_parameters()}}
    refs = {}
    for tag, dtype in (('o64', torch.float64), ('o32', torch.float32)):
        o = WU.seg_oracle(gold, dtype, loss_type, w, gamma, fa, smooth, weights=sd)
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
    print(f'{name} {loss_type} weights {w}: worst error {worst:.3f} of its bound')
    # ... and the weights do change the step: the unweighted oracle's generator gradient is another one
    plain = U.seg_oracle(gold, torch.float64, loss_type, gamma, fa, smooth) if sd is None else None
    if plain is not None:
        plain.batch(x, y, train=True)
        k = next(iter(plain.last['g_grads']))
        assert _l2(plain.last['g_grads'][k], refs['o64']['g_grads'][k]) > 1e-2
    t.release()


_MODE_RUNS = {}


def _mode_run(tmp_path_factory, mode):
    if mode not in _MODE_RUNS:
        gold = Golden(SOFTMAX)
        g, d = _nets(gold)
        x, y = gold.inputs()
        t = _trainer(g, d, tmp_path_factory.mktemp('segw_mode'), 'ce+dice', mode=mode, class_weights=W4)
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


def test_changed_weights_are_another_kind_of_step(tmp_path):
    """The weights' buffer is a launch argument: a captured step holds the one it was captured with.  After six steps with one set of
    weights (three of them replays) the attribute changes: the next step is another kind -- launched eagerly again, captured again
    after its warm steps -- and its losses are, bit for bit, those of a trainer that never captured anything and changed the weights at
    the same step.  Back to the first weights: the first capture replays again."""
    gold = Golden(SOFTMAX)
    x, y = gold.inputs()
    other = [2.0, 0.5, 1.0, 0.25]
    runs = {}
    for mode in ('graph', 'eager1'):
        g, d = _nets(gold)
        t = _trainer(g, d, tmp_path / mode, 'ce+dice', mode=mode, class_weights=list(W4))
        rows, modes = [], []
        for s in range(2 * STEPS + 2):
            if s == STEPS:
                t.class_weights = other
            if s == 2 * STEPS:
                t.class_weights = tuple(W4)
            rows.append(_row(t.batch(x, y, train=True)))
            modes.append(t.launch_mode)
        t.flush()
        torch.cuda.synchronize()
        runs[mode] = (np.array(rows), modes, g.flat.cpu().numpy().copy())
        t.release()
    rows, modes, gw = runs['graph']
    assert modes[3:STEPS] == ['graph'] * (STEPS - 3) and modes[STEPS] != 'graph' and modes[STEPS + 3:] == ['graph'] * (STEPS - 1), modes
    assert np.array_equal(rows, runs['eager1'][0]) and np.array_equal(gw, runs['eager1'][2])
    # ... and the weights do change the objective: with the first set kept throughout, step 7 reports another loss
    g, d = _nets(gold)
    t = _trainer(g, d, tmp_path / 'kept', 'ce+dice', mode='eager1', class_weights=W4)
    kept = np.array([_row(t.batch(x, y, train=True)) for _ in range(STEPS + 1)])
    t.release()
    assert np.array_equal(kept[:STEPS], rows[:STEPS]) and kept[STEPS, 0] != rows[STEPS, 0]


SEG_OFF = ('pg_seg_loss_workspace_bytes', 'pg_seg_loss_reduce', 'pg_seg_loss_value_grad')


def test_off_is_off(tmp_path, monkeypatch):
    """class_weights = None set explicitly against a trainer whose attribute was never touched: the same library calls with the same
    arguments -- pg_seg_loss_value_grad, never pg_seg_loss_value_grad_w or pg_seg_label_count --, the same losses and weights bit for
    bit.  With weights: pg_seg_loss_value_grad_w in its place with the same scalar arguments, once per step, and every other call
    unchanged."""
    never = _recorded(tmp_path, monkeypatch, 'never', SOFTMAX, loss_type='ce+dice')
    off = _recorded(tmp_path, monkeypatch, 'off', SOFTMAX, loss_type='ce+dice', class_weights=None, class_weight_batches=3)
    on = _recorded(tmp_path, monkeypatch, 'on', SOFTMAX, loss_type='ce+dice', class_weights=W4)
    ones = _recorded(tmp_path, monkeypatch, 'ones', SOFTMAX, loss_type='ce+dice', class_weights=[1, 1, 1, 1])
    for a, b in zip(never[:3], off[:3]):
        assert np.array_equal(a, b)
    assert never[3].calls == off[3].calls and len(never[3].calls) > 100
    assert all(never[3].names.count(n) == 3 for n in SEG_OFF)
    assert not any(n in ('pg_seg_loss_value_grad_w', 'pg_seg_label_count') for n in never[3].names)
    names = on[3].names
    assert names.count('pg_seg_loss_value_grad_w') == 3 and names.count('pg_seg_loss_value_grad') == 0 and names.count('pg_seg_loss_reduce') == 3
    swap = lambda rec: [(('pg_seg_loss_value_grad',) + c[1:2] if c[0] == 'pg_seg_loss_value_grad_w' else c[:2]) for c in rec.calls]
    assert swap(on[3]) == swap(never[3])          # (the same entry points with the same scalar arguments in the same order)
    assert not np.array_equal(on[0], never[0])
    # all-ones weights: the weighted entry point, the unweighted bits
    assert ones[3].names.count('pg_seg_loss_value_grad_w') == 3
    for a, b in zip(never[:3], ones[:3]):
        assert np.array_equal(a, b)


def test_evaluation_uses_the_weights_and_updates_nothing(tmp_path, monkeypatch):
    """batch(train=False) and evaluate() with weights: pg_seg_loss_value_grad_w without a gradient, no Adam launch, no weight of either
    network changed; the value against the weighted float64 oracle within 8 x the fp32 oracle's own distance + 1e-5 (relative), and not
    the unweighted value.  Measured on an MI355X: the evaluation step within 1.2e-08, evaluate() within 4.5e-09 (bound 1.0e-05)."""
    gold = Golden(SOFTMAX)
    x, y = gold.inputs()
    g, d = _nets(gold)
    g0, d0 = g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy()
    rows, g1, d1, rec = _recorded(tmp_path, monkeypatch, 'eval', SOFTMAX, nsteps=1, train=False, loss_type='ce+dice', class_weights=W4)
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    assert rec.names.count('pg_seg_loss_reduce') == 1 and rec.names.count('pg_seg_loss_value_grad_w') == 1 and rec.names.count('pg_seg_loss_value_grad') == 0
    assert not any(n.startswith('pg_adam') for n in rec.names)
    o64, o32 = (WU.seg_oracle(gold, dt, 'ce+dice', W4) for dt in (torch.float64, torch.float32))
    o64.batch(x, y, train=False)
    o32.batch(x, y, train=False)
    plain = U.seg_oracle(gold, torch.float64, 'ce+dice')
    plain.batch(x, y, train=False)
    want, noise = o64.last['seg'], abs(o32.last['seg'] - o64.last['seg']) / abs(o64.last['seg'])
    bound = 8 * noise + 1e-5
    assert abs(plain.last['seg'] - want) > 1e-2 * abs(want)
    t = _trainer(g, d, tmp_path / 'evaluate', 'ce+dice', class_weights=W4)
    seg_step = float(t.batch(x, y, train=False)['gen']) - float(t.batch(x, y, train=False)['gdisc'])
    out = t.evaluate([(x, y), (x, y)])
    for what, got in (('evaluation step (gen - gdisc)', seg_step), ('evaluate()', out['seg_loss'])):
        e = abs(got - want) / abs(want)
        print(f'weighted ce+dice {what}: seg_loss {got:.8f} oracle {want:.8f} rel {e:.2e} (bound {bound:.2e})')
        assert e <= bound + (1e-6 if what.startswith('evaluation step') else 0.0), (what, e)
    assert np.array_equal(g.flat.cpu().numpy(), g0) and np.array_equal(d.flat.cpu().numpy(), d0)
    t.release()


def _imbalanced_batches(nbatches, N, cfg, seed):
    """(x, y) batches whose one-hot targets are heavily imbalanced, with one class absent and some pixels unlabelled."""
    C, size = cfg['out_nc'], cfg['size']
    assert C == 4
    gen = torch.Generator().manual_seed(seed)
    probs = torch.tensor([0.85, 0.1, 0.0, 0.05])
    out = []
    for _ in range(nbatches):
        labels = torch.multinomial(probs, N * size * size, replacement=True, generator=gen).reshape(N, size, size)
        y = torch.nn.functional.one_hot(labels, C).permute(0, 3, 1, 2).float()
        y = y * (torch.rand(N, 1, size, size, generator=gen) > 0.1)
        out.append((torch.rand(N, cfg['in_nc'], size, size, generator=gen), y.contiguous()))
    return out


def _np_counts(batches):
    return sum(WU.label_counts(y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1]).numpy()) for _, y in batches)


def test_estimate_class_weights_and_its_file(tmp_path):
    """estimate_class_weights on an in-memory loader: the counts are NumPy's, the weights class_weights_from_counts of them (both
    schemes, max_batches), set on the trainer and usable by the next step; class_weights.json round-trips through
    load_last_checkpoint() of a new trainer whose setting is the scheme's name, which then does not estimate again."""
    from patchgan_amd import engine as E
    gold = Golden(SOFTMAX)
    c = gold.cfg
    g, d = _nets(gold)
    data = _imbalanced_batches(3, 2, c, 5)
    t = _trainer(g, d, tmp_path, 'ce+dice')
    for scheme, nb in (('balanced_sqrt', 2), ('balanced', None)):
        want = _np_counts(data[:nb])
        got = t.estimate_class_weights(data, scheme, max_batches=nb)
        info = t.class_weight_info
        assert info['counts'] == want[:4].tolist() and info['unlabelled'] == want[4] and info['pixels'] == want[5] and want[2] == 0 and want[4] > 0
        assert got == E.class_weights_from_counts(want[:4], scheme) == t.class_weights == info['weights'] and info['scheme'] == scheme
        assert json.load(open(tmp_path / 'class_weights.json')) == info
    assert got[1] > 5 * got[0] and got[2] == max(got)
    first = _row(t.batch(*data[0], train=True))
    assert np.isfinite(first).all()
    t.save(1)
    t.release()
    g2, d2 = _nets(gold)
    t2 = _trainer(g2, d2, tmp_path, 'ce+dice', class_weights='balanced')
    with pytest.raises(ValueError):
        t2.batch(*data[0], train=True)          # (a scheme's name that nothing has resolved yet)
    t2.load_last_checkpoint()
    assert t2.class_weights == got and t2.class_weight_info == info and t2.start == 2
    assert np.isfinite(_row(t2.batch(*data[0], train=False))).all()
    t2.release()


def test_train_estimates_before_the_first_epoch(tmp_path, capsys):
    gold = Golden(SOFTMAX)
    c = gold.cfg
    g, d = _nets(gold)
    data = _imbalanced_batches(2, 2, c, 6)
    t = _trainer(g, d, tmp_path, 'ce+dice', class_weights='balanced', class_weight_batches=1)
    t.train(data, data[:1], 1, save_freq=10)
    want = _np_counts(data[:1])
    assert t.class_weight_info['counts'] == want[:4].tolist() and isinstance(t.class_weights, list)
    assert 'Class weights (balanced)' in capsys.readouterr().out and os.path.exists(tmp_path / 'class_weights.json')
    t.release()


def _dp_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    import tempfile
    from patchgan_amd.parallel import shard_batch
    gold = Golden(SOFTMAX)
    g, d = _nets(gold)
    data = _imbalanced_batches(2, 2, gold.cfg, 7)
    t = _trainer(g, d, tempfile.mkdtemp(), 'ce+dice')
    w = t.estimate_class_weights([shard_batch(x, y, rank, world) for x, y in data], 'balanced')
    xs, ys = shard_batch(*data[0], rank, world)
    row = _row(t.batch(xs, ys, train=True))
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, w, t.class_weight_info['counts'], np.array(row), g.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_against_the_single_process(tmp_path):
    """Two ranks (gloo, both on the one GPU), each with half of every batch: the estimate over the two shards is the single process's
    exactly (integer counts, one all-reduce), and one weighted ce+dice step matches the single process on the whole batch within the
    bound of test_segloss_gpu.py::test_two_ranks_against_the_single_process (losses to 1e-4 relative).  Measured on an MI355X: the six
    losses equal the single process's bit for bit."""
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    gold = Golden(SOFTMAX)
    g, d = _nets(gold)
    data = _imbalanced_batches(2, 2, gold.cfg, 7)
    t = _trainer(g, d, tmp_path, 'ce+dice')
    w = t.estimate_class_weights(data, 'balanced')
    counts = t.class_weight_info['counts']
    single = np.array(_row(t.batch(*data[0], train=True)))
    t.release()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, w0, c0, r0, g0), (_, w1, c1, r1, g1) = res
    assert w0 == w1 == w and c0 == c1 == counts
    assert np.array_equal(g0, g1) and np.allclose(r0, r1, rtol=1e-6)
    err = np.abs(r0 - single) / np.maximum(np.abs(single), 1e-6)
    print('weighted ce+dice dp2 vs single process: rel err', err)
    assert err.max() < 1e-4, err


def test_every_option_together_on_bf16_networks(tmp_path):
    """Weights with accumulation, clipping, the weight average and bf16 networks: four calls (two optimizer steps) stay finite and move
    the weights and the average."""
    torch.manual_seed(3)
    gold = Golden(SOFTMAX)
    g, d = _nets(gold, nf=16, ndf=32)
    g.set_precision('bf16')
    d.set_precision('bf16')
    x, y = gold.inputs()
    t = _trainer(g, d, tmp_path, 'ce+focal+dice', 2, 0.25, 1.0, class_weights=W4, accumulate=2, clip_grad_norm=1.0, ema_decay=0.99)
    g0, e0 = g.flat.cpu().numpy().copy(), t.ema_generator.flat.cpu().numpy().copy()
    rows = [_row(t.batch(x, y, train=True)) for _ in range(4)]
    t.flush()
    torch.cuda.synchronize()
    assert np.isfinite(rows).all(), rows
    assert torch.isfinite(g.flat).all() and torch.isfinite(d.flat).all() and torch.isfinite(t.ema_generator.flat).all()
    assert not np.array_equal(g.flat.cpu().numpy(), g0) and not np.array_equal(t.ema_generator.flat.cpu().numpy(), e0)
    stats = t.read_grad_stats()
    assert stats['gen']['steps'] == 2 and stats['gen']['skipped'] == 0 and stats['disc']['skipped'] == 0 and (t._t_g, t._t_d) == (2, 2)
    t.release()
