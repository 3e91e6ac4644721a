"""D(x | G(x)) once per step (Trainer SHARE_D_FAKE): the discriminator's 2N pass run as two N-sample half passes that fill one context.

Every comparison is torch.equal / array_equal: zero tolerance.  The conv cases check the C ABI (pg_conv_extras.v_stride / v_tile0): two
half calls write the halves of the whole call's output and of its kept transform V[point][tile][k], and nothing else; the step cases
check that a training run with the shared pass IS the run with the reference's three passes.  Needs an MI355X.

Shapes.  A kept V exists where forward AND weight gradient take a Winograd path, and the gates are tile counts: the polyphase weight
gradient needs >= 512 tiles, the 128-row GEMM tile starts at 1024 tiles, the stride-1 path needs N * ceil(H/2) * ceil(W/2) >= 2048.
So (op.describe confirms each, see _case):
  s2-128   2N = 18, 72x72 -> 36x36 (144 tiles per sample): 1296 tiles per half = 10.125 x 128, the 128-row tile at N and at 2N, V kept.
           (2N = 8 on this map puts the halves on the 64-row tile and the whole on the 128-row tile: not "the same kernel".)
  s2-64    2N = 10, 20x20 -> 10x10 (16 tiles per sample): 80 tiles per half = 1.25 x 64, the 64-row tile at N and at 2N.  No weight
           gradient on this path below 512 tiles, hence no kept V: the outputs are compared.  (2N = 6 leaves the half under the
           polyphase path's 64-tile minimum: another kernel family at N than at 2N.)
  s2-64v   2N = 66 on the same map: 528 tiles per half = 8.25 x 64, the 64-row tile WITH a kept, strided V.  The whole call runs the
           128-row tile here, so V is compared with the whole call's and the outputs with dense half calls.
  s1-row   2N = 64, 17x17 -> 16x16, F(3x3,4x4) pinned: 1152 tiles per half = 9 x 128 for the split-bf16 row GEMM, 18 x 64 for the
           fp32 one; a sample boundary every 36 rows.  (2N = 4 is under the stride-1 gate: implicit GEMM.)
"""
import numpy as np
import pytest
import torch

from tests.golden_util import LOSS_KEYS

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _algo(kind, s3off):
    from patchgan_amd import _lib as L
    a = L.ALGO_AUTO | (L.TUNE_WINO1_F3 if kind == 's1' else L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL)
    return a | (L.TUNE_S3_OFF if s3off else 0)


# name -> (2N, big extent, stride kind, symbol family with / without PG_TUNE_S3_OFF, V kept, halves == whole by the planner)
CASES = {
    's2-128': (18, 72, 's2', ('k_wino_bgemm_s3<2,2,2,2,2>', 'k_wino_bgemm<2,2,2,2>'), True, True),
    's2-64': (10, 20, 's2', ('k_wino_bgemm_s3<1,2,2,2,3>', 'k_wino_bgemm<1,2,2,2>'), False, True),
    's2-64v': (66, 20, 's2', ('k_wino_bgemm_s3<1,2,2,2,3>', 'k_wino_bgemm<1,2,2,2>'), True, False),
    's1-row': (64, 17, 's1', ('k_wino_gemm_row_s3<2>', 'k_wino_gemm_row<4,1>'), True, True),
}


def _case(name, Ca, s3off):
    """(half op, whole op, operands) of one case; asserts the planner picks the intended kernels."""
    from patchgan_amd import engine as E
    N2, Hb, kind, syms, keeps, same = CASES[name]
    algo = _algo(kind, s3off)
    stride = 1 if kind == 's1' else 2
    half, whole = E.ConvOp(N2 // 2, Hb, Hb, Ca, 64, stride, algo), E.ConvOp(N2, Hb, Hb, Ca, 64, stride, algo)
    assert half.describe(0) == (syms[1 if s3off else 0], 1), half.describe(0)
    assert bool(half.v_bytes()) == bool(whole.v_bytes()) == keeps
    assert half.halves_same(whole) == same
    if same:
        assert whole.describe(0) == half.describe(0)
    g = torch.Generator().manual_seed(11)
    big = E.View.alloc(N2, Hb, Hb, 64, 'cuda')
    big.t.copy_(torch.randn(big.t.numel(), generator=g))
    P = torch.randn(16 * Ca * 64 + Ca, generator=g).cuda() * 0.05
    return half, whole, big, P


def _fwd(op, big, P, small, v, v_part=(0, 0)):
    from patchgan_amd import _lib as L
    op.big2small(big, P, 0, P, 16 * op.Ca * op.Cb, small, L.ACT_TANH, v_keep=v, v_part=v_part)


def _nan_view(N, H, W, C):
    from patchgan_amd import engine as E
    v = E.View.alloc(N, H, W, C, 'cuda')
    v.t.fill_(NAN)
    return v


def _nan_v(op):
    return torch.full((op.v_bytes() // 4,), NAN, dtype=torch.float32, device='cuda') if op.v_bytes() else None


def _planes(op, whole, v):
    """v as [points][tiles of the whole batch][k]"""
    stride, _ = op.v_part(whole, 0)
    pts = 16 if op.stride == 2 else 36
    return v[:pts * stride].view(pts, whole.N, stride // whole.N)


def _halves(half, whole, big, P):
    """Output and V of the whole batch written by two half calls, with the containment checks after the first."""
    N = half.N
    out, v = _nan_view(whole.N, whole.Hs, whole.Ws, whole.Ca), _nan_v(whole)
    for first, n0 in enumerate((N, 0)):                       # the fake half first, as the step does
        _fwd(half, big.samples(n0, N), P, out.samples(n0, N), v, half.v_part(whole, n0) if v is not None else (0, 0))
        torch.cuda.synchronize()
        if first == 0:
            o = out.t.view(whole.N, -1)
            assert not torch.isnan(o[N:]).any() and torch.isnan(o[:N]).all(), 'the first half call wrote outside its half of the output'
            if v is not None:
                p = _planes(half, whole, v)
                assert not torch.isnan(p[:, N:]).any() and torch.isnan(p[:, :N]).all(), 'the first half call wrote outside its rows of V'
    return out, v


@pytest.mark.parametrize('s3off', [False, True], ids=['s3', 'fp32mfma'])
@pytest.mark.parametrize('Ca', [64, 128])
@pytest.mark.parametrize('name', list(CASES))
def test_half_calls_equal_the_whole_call_and_stay_inside_their_half(name, Ca, s3off):
    half, whole, big, P = _case(name, Ca, s3off)
    ref_out, ref_v = _nan_view(whole.N, whole.Hs, whole.Ws, whole.Ca), _nan_v(whole)
    _fwd(whole, big, P, ref_out, ref_v)
    out, v = _halves(half, whole, big, P)
    torch.cuda.synchronize()
    assert not torch.isnan(ref_out.t).any()
    if ref_v is not None:
        assert not torch.isnan(ref_v).any()
        assert torch.equal(v, ref_v), 'V of the two half calls != V of the whole call'
    if CASES[name][5]:
        assert torch.equal(out.t, ref_out.t), 'output of the two half calls != output of the whole call'
    else:
        # the whole call runs another GEMM tile here (the planner says so): the strided rows against the same plan on dense buffers
        N = half.N
        for n0 in (0, N):
            d_out, d_v = _nan_view(N, half.Hs, half.Ws, half.Ca), _nan_v(half)
            _fwd(half, big.samples(n0, N), P, d_out, d_v)
            torch.cuda.synchronize()
            assert torch.equal(out.samples(n0, N).t[out.samples(n0, N).off:][:d_out.t.numel()], d_out.t)
            assert torch.equal(_planes(half, whole, v)[:, n0:n0 + N].reshape(-1), d_v[:v.numel() // 2])


@pytest.mark.parametrize('name', ['s2-128', 's1-row'])
def test_weight_gradient_from_a_v_assembled_by_half_calls(name):
    from patchgan_amd import engine as E
    Ca = 128
    half, whole, big, P = _case(name, Ca, False)
    assert whole.describe(2)[0].startswith('k_wino_wgrad_gemm')
    ref_out, ref_v = _nan_view(whole.N, whole.Hs, whole.Ws, Ca), _nan_v(whole)
    _fwd(whole, big, P, ref_out, ref_v)
    out, v = _halves(half, whole, big, P)
    dy = E.View.alloc(whole.N, whole.Hs, whole.Ws, Ca, 'cuda')
    dy.t.copy_(torch.randn(dy.t.numel(), generator=torch.Generator().manual_seed(12)))
    grads = []
    for vv in (ref_v, v):
        dP = torch.full((16 * Ca * 64 + Ca,), NAN, device='cuda')
        whole.wgrad(dy, big, dP, 0, dP, 16 * Ca * 64, v_pre=vv.view(torch.uint8))
        grads.append(dP)
    torch.cuda.synchronize()
    assert not torch.isnan(grads[0]).any()
    assert torch.equal(grads[0], grads[1])


def test_part_fields_are_validated():
    """A range that leaves its plane, a stride without a kept V and the fields on the other entry points are refused (PG_EINVAL,
    nothing launched)."""
    half, whole, big, P = _case('s2-128', 64, False)
    N = half.N
    out, v = _nan_view(whole.N, whole.Hs, whole.Ws, 64), _nan_v(whole)
    stride, tile0 = half.v_part(whole, N)
    for bad in ((stride, tile0 + 1), (stride // 2 - 4, 0), (stride + 2, 0), (-stride, 0), (stride, -1), (0, 4)):
        with pytest.raises(RuntimeError, match='PG_EINVAL'):
            _fwd(half, big.samples(N, N), P, out.samples(N, N), v, bad)
    torch.cuda.synchronize()
    assert torch.isnan(out.t).all() and torch.isnan(v).all()


# ------------------------------------------------------------------------------------------------ the step
def _trainer(tmp_path, tag, N, mode, norm_layer=None, train=True):
    import patchgan_amd as pg
    torch.manual_seed(5)
    g = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 64, n_layers=3) if norm_layer is None else pg.Discriminator(4, 64, n_layers=3, norm=True, norm_layer=norm_layer)
    g.cuda(), d.cuda()
    t = pg.Trainer(g, d, str(tmp_path / tag))
    if mode == 'graph':
        t.graph, t.GRAPH_WARM_STEPS = True, 1
    elif mode == 'eager2':
        t.two_streams = True
    t.setup_optimizers(1e-3, 2e-3)
    g.train(train), d.train(train)
    return g, d, t


def _steps(tmp_path, monkeypatch, share, N, mode, steps=3, norm_layer=None, train=True, count=False):
    from patchgan_amd import trainer as T, engine as E
    monkeypatch.setattr(T, 'SHARE_D_FAKE', share)
    g, d, t = _trainer(tmp_path, f'{mode}_{share}_{N}', N, mode, norm_layer, train)
    gen = torch.Generator().manual_seed(6)
    rows, launches = [], []
    for s in range(steps):
        x = torch.rand(N, 3, 256, 256, generator=gen)
        y = (torch.rand(N, 1, 256, 256, generator=gen) > 0.7).float()
        if count:
            monkeypatch.setattr(E, 'PROFILER', E.LaunchProfiler())
        l = t.batch(x, y, train=train)
        rows.append([float(l[k]) for k in LOSS_KEYS])
        if count:
            launches.append((len(E.PROFILER.records), sum(r[2] for r in E.PROFILER.records)))      # launches, algorithmic FLOPs
            monkeypatch.setattr(E, 'PROFILER', None)
    t.flush()
    torch.cuda.synchronize()
    out = (np.array(rows), g.flat.cpu().numpy().copy(), d.flat.cpu().numpy().copy(), launches, t.launch_mode)
    t.release()
    return out


N_SHARED = 9       # the smallest batch at 256x256 / ndf = 64 at which every D layer runs the same kernel at N and 2N (d2: 1089 tiles)


@pytest.mark.parametrize('mode', ['eager1', 'eager2', 'graph'])
def test_training_steps_are_the_three_pass_steps(tmp_path, monkeypatch, mode):
    from patchgan_amd import engine as E
    de = E.DiscriminatorEngine(4, 64, 3, False)
    assert de.halves_ok(N_SHARED, 256, 256)
    syms = [op.describe(0)[0].split('<')[0] for op in de.ops(N_SHARED, 256, 256)]
    assert 'k_wino_bgemm_s3' in syms and 'k_wino_gemm_row_s3' in syms, syms
    steps = 4 if mode == 'graph' else 3          # (the capture replaces the third step of its kind)
    a = _steps(tmp_path, monkeypatch, False, N_SHARED, mode, steps)
    b = _steps(tmp_path, monkeypatch, True, N_SHARED, mode, steps)
    assert a[4] == b[4] == mode, (a[4], b[4])
    assert np.array_equal(a[0], b[0]), a[0] - b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize('mode', ['eager1', 'eager2'])
def test_evaluation_steps_are_the_three_pass_steps(tmp_path, monkeypatch, mode):
    a = _steps(tmp_path, monkeypatch, False, N_SHARED, mode, 2, train=False)
    b = _steps(tmp_path, monkeypatch, True, N_SHARED, mode, 2, train=False)
    assert np.array_equal(a[0], b[0]), a[0] - b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_shared_step_runs_one_n_sample_forward_pass_less(tmp_path, monkeypatch):
    """engine.LaunchProfiler over a step.  The three-pass step makes its three passes in TWO sets of launches (N samples, then real and
    fake as one 2N batch); the shared step makes two sets of N samples.  So the number of conv launches is the same -- the 2N launches
    become N launches -- and what the step no longer does is exactly one N-sample forward pass: its algorithmic FLOPs (integers held
    exactly in doubles) are lower by the five layers' N-sample counts."""
    from patchgan_amd import engine as E
    a = _steps(tmp_path, monkeypatch, False, N_SHARED, 'eager1', 2, count=True)
    b = _steps(tmp_path, monkeypatch, True, N_SHARED, 'eager1', 2, count=True)
    one_pass = sum(op.flops for op in E.DiscriminatorEngine(4, 64, 3, False).ops(N_SHARED, 256, 256))
    assert one_pass > 0
    for (la, fa), (lb, fb) in zip(a[3], b[3]):
        assert la == lb and fa - fb == one_pass, (la, lb, fa - fb, one_pass)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize('what', ['batchnorm', 'plans-differ'])
def test_fallbacks_keep_three_passes(tmp_path, monkeypatch, what):
    """A BatchNorm discriminator, and a batch whose N and 2N plans differ (N = 2: d1 on the 64-row tile at N, the 128-row tile at 2N;
    the planner predicate is False, tests/test_share_dfake_cpu.py), run the three passes whatever the switch says."""
    from patchgan_amd import engine as E
    import torch.nn as nn
    if what == 'plans-differ':
        assert not E.DiscriminatorEngine(4, 64, 3, False).halves_ok(2, 256, 256)
    kw = dict(norm_layer=nn.BatchNorm2d) if what == 'batchnorm' else {}
    N = 4 if what == 'batchnorm' else 2
    a = _steps(tmp_path, monkeypatch, False, N, 'eager1', 2, count=True, **kw)
    b = _steps(tmp_path, monkeypatch, True, N, 'eager1', 2, count=True, **kw)
    assert a[3] == b[3] and a[3][0][0] > 0, (a[3], b[3])      # the same launches and the same FLOPs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
