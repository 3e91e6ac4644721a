"""The inputs of tests/test_exact_gpu.py discriminate, shown without a GPU: their exactness budget holds at every geometry the GPU
file uses, float64 and fp32 convolution agree exactly on them, a NumPy fp32 model of the split-bf16 polyphase Winograd path
reproduces the float64 result bit for bit under a random summation order -- and stops doing so when any one of the six products
a_i b_j is dropped."""
import os
import random

import numpy as np
import pytest
import torch

from tests import exact_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_GEOM = (2, 10, 14, 8, 8, 2)         # Hs x Ws = 5 x 7: 2 x 3 tiles per sample, ragged in both directions; K = 32: two chunks
SPLIT = {'s3': 0, 'fp32': 1}


def _gpu_cases():
    """(geometry, opcode, budget path) of every fp32-tensor case of the GPU file, from the planner's own answers (host-side queries)."""
    from patchgan_amd import engine as E
    from tests import test_exact_gpu as G
    for geom, algo in G.all_fp32_cases():
        op = E.ConvOp(*geom, algo)
        for opcode in range(3):
            yield geom, opcode, op.describe(opcode)[0]


def test_tables_are_the_kernels_and_dyadic():
    src = X.source_tables(os.path.join(ROOT, 'patchgan_amd', 'csrc', 'conv_wino.hip'))
    for name, t in X.TABLES.items():
        assert np.array_equal(src[name], t), name
        assert set(np.abs(t).ravel().tolist()) <= {0.0, 0.5, 1.0}, name
    assert (X.GAIN_IN, X.GAIN_W, X.TERMS_OUT, X.GAIN_DY, X.TERMS_OUT_W) == (4.0, 1.0, 9, 2.25, 9)


def test_budget_holds_for_every_gpu_geometry():
    worst = {}
    for geom, opcode, sym in _gpu_cases():
        r = X.budget_for(X.exact_operands(geom), opcode, sym)        # raises where a geometry is not provably exact
        path = X.path_of(sym, geom[5])
        worst[path] = max(worst.get(path, 0.0), r)
    print('largest worst-case / lsb ratios (log2):', {k: round(float(np.log2(v)), 2) for k, v in worst.items()})
    assert set(worst) == {'gemm', 'wino2', 'wino2w'}
    from tests import test_exact_gpu as G
    for geom in G.WINO2_GEOMS:
        for op in (0, 1):
            for shape in X.WIDE:
                X.wide_budget(X.wide_conv_operands(geom, op, shape), op)
    for geom in G.WINO2W_GEOMS:
        for shape in X.WIDE:
            X.wide_budget(X.wide_wgrad_operands(geom, shape), 2)


def test_budget_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):          # 16-bit activations against dense weights
        X.assert_exact_budget((4, 32, 32, 128, 64, 2), 0, 'wino2', 1.0, 2.0, 2.0 ** -16, 1.0)
    with pytest.raises(AssertionError):          # 16-bit values on both sides: 32-bit products
        X.assert_exact_budget(MODEL_GEOM, 0, 'wino2', 1.0, 1.0, 2.0 ** -16, 2.0 ** -16, terms=1)
    with pytest.raises(AssertionError):
        X.path_of('k_wino_gemm<2,1,2,2,2,2>', 1)
    with pytest.raises(AssertionError):
        X.to_fp32_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


@pytest.mark.parametrize('geom', [(2, 16, 16, 64, 32, 2), (3, 12, 20, 36, 20, 2), (2, 9, 9, 8, 8, 1), (2, 4, 4, 512, 64, 2), (1, 15, 13, 3, 20, 2)],
                         ids=lambda g: 'x'.join(map(str, g)))
def test_float64_equals_fp32_convolution_on_exact_operands(geom):
    """torch's fp32 CPU kernels (another summation order again) give the float64 result exactly; one weight changed by its least
    significant bit changes the reference (the generator is not degenerate)."""
    import torch.nn.functional as F
    ops = X.exact_operands(geom)
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    for t, lo, hi in ((ops.big, -3, 3), (ops.small, -3, 3), (ops.Wt, -2, 2)):
        assert t.min() == lo and t.max() == hi and torch.equal(t, t.round()) and torch.equal(t, t.bfloat16().float())
    for act in ('none', 'relu'):
        w0 = X.to_fp32_exact(X.reference64(ops, 0, act))
        w1 = X.to_fp32_exact(X.reference64(ops, 1, act))
        f = (lambda t: t.clamp_min(0)) if act == 'relu' else (lambda t: t)
        assert torch.equal(f(F.conv2d(ops.big, ops.Wt, ops.bias_a, stride=s, padding=1)), w0)
        opad = (Hb - ((Hs - 1) * s + 2), Wb - ((Ws - 1) * s + 2))
        assert torch.equal(f(F.conv_transpose2d(ops.small, ops.Wt, ops.bias_b, stride=s, padding=1, output_padding=opad)), w1)
    dW, db = X.reference64(ops, 2)
    assert torch.equal(torch.nn.grad.conv2d_weight(ops.big, (Ca, Cb, 4, 4), ops.small, stride=s, padding=1), X.to_fp32_exact(dW))
    assert torch.equal(ops.small.sum((0, 2, 3)), X.to_fp32_exact(db))
    nudged = X.Operands(geom, ops.big, ops.small, ops.Wt.clone(), ops.bias_a, ops.bias_b)
    nudged.Wt[Ca // 2, Cb // 2, 1, 2] += 1.0
    assert not torch.equal(X.reference64(nudged, 0), X.reference64(ops, 0)) and not torch.equal(X.reference64(nudged, 1), X.reference64(ops, 1))


def test_bf16_rounding_and_split_of_the_model():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    x = torch.cat([x, torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0])])      # ties, both ways
    assert np.array_equal(X.bf16_rne(x.numpy()), x.bfloat16().float().numpy())
    h, m, l = X.s3_split(x.numpy())
    assert np.array_equal((h.astype(np.float64) + m + l).astype(np.float32), x.numpy())       # 8 + 8 + 8 bits cover fp32's 24


def _fwd_cases():
    yield 'int', X.exact_operands(MODEL_GEOM)
    for shape in X.WIDE:
        yield shape, X.wide_conv_operands(MODEL_GEOM, 0, shape)


def _pieces(t):
    """How many of the three bf16 pieces some element of t needs."""
    h, m, l = X.s3_split(np.asarray(t, np.float32))
    return 3 if l.any() else 2 if m.any() else 1


def test_model_reproduces_float64_and_every_product_matters():
    """Forward path.  Exact under a random summation order for the small-integer case and each wide case; each of the six products,
    when dropped, changes the result of at least one wide case."""
    seen = {}
    V_pieces = {}
    for name, ops in _fwd_cases():
        want = X.to_fp32_exact(X.reference64(ops, 0, bias=False)).numpy()
        if name == 'int':
            X.assert_exact_budget(MODEL_GEOM, 0, 'wino2', ops.amax[0], ops.amax[2])
        else:
            X.wide_budget(ops, 0)
        for seed in (None, 1, 2):
            rng = random.Random(seed) if seed is not None else None
            got = X.polyphase_fwd_model(ops.big, ops.Wt, lambda a, b: X.s3_model(a, b, rng=rng))
            assert np.array_equal(got, want), (name, seed, np.abs(got - want).max())
        for p in X.S3_PRODUCTS:
            got = X.polyphase_fwd_model(ops.big, ops.Wt, lambda a, b: X.s3_model(a, b, drop=p))
            seen[name, p] = not np.array_equal(got, want)
        V = X._phase_windows(ops.big.numpy(), 2, 3)
        V_pieces[name] = _pieces(V)
    print({k: v for k, v in seen.items() if v})
    assert V_pieces == {'int': 1, '3,1': 3, '1,3': 1, '2,2': 2}, V_pieces       # the transformed values need the pieces their name says
    assert [p for p in X.S3_PRODUCTS if seen['int', p]] == [(0, 0)]            # small integers never leave the first piece
    assert seen['3,1', (0, 0)] and seen['3,1', (1, 0)] and seen['3,1', (2, 0)]
    assert seen['1,3', (0, 0)] and seen['1,3', (0, 1)] and seen['1,3', (0, 2)]
    assert seen['2,2', (1, 1)]
    for p in X.S3_PRODUCTS:
        assert any(seen[name, p] for name in X.WIDE), p


def test_model_weight_gradient_wide_cases():
    """The transposed construction: dW is a gather of `big`, exact in the model under a random order, the transformed dy is no
    larger than dy (the unit gain the budget assumes), and every product matters in some case."""
    seen = {}
    for shape in X.WIDE:
        ops = X.wide_wgrad_operands(MODEL_GEOM, shape)
        X.wide_budget(ops, 2)
        assert ((ops.small != 0).sum((0, 2, 3)) == (4 if X.WIDE[shape][1] else 1)).all()
        want = X.to_fp32_exact(X.reference64(ops, 2)[0]).numpy()
        assert np.count_nonzero(want) > want.size // 4
        rng = random.Random(5)
        got, DY = X.polyphase_wgrad_model(ops.big, ops.small, lambda a, b: X.s3_model(a, b, rng=rng))
        assert np.array_equal(got, want), (shape, np.abs(got - want).max())
        assert np.abs(DY).max() <= ops.amax[1]
        for p in X.S3_PRODUCTS:
            seen[shape, p] = not np.array_equal(X.polyphase_wgrad_model(ops.big, ops.small, lambda a, b: X.s3_model(a, b, drop=p))[0], want)
    for p in X.S3_PRODUCTS:
        assert any(seen[shape, p] for shape in X.WIDE), p
    ops = X.exact_operands(MODEL_GEOM)
    X.assert_exact_budget(MODEL_GEOM, 2, 'wino2w', ops.amax[1], ops.amax[0])
    got, _ = X.polyphase_wgrad_model(ops.big, ops.small, lambda a, b: X.s3_model(a, b, rng=random.Random(9)))
    assert np.array_equal(got, X.to_fp32_exact(X.reference64(ops, 2)[0]).numpy())


def test_existing_bounds_cannot_see_a_dropped_third_order_product():
    """Why zero tolerance: on the data built to expose it, losing a3 b1 moves the max-norm by less than the suite's 2e-5 bound."""
    ops = X.wide_conv_operands(MODEL_GEOM, 0, '3,1')
    want = X.reference64(ops, 0, bias=False).numpy()
    got = X.polyphase_fwd_model(ops.big, ops.Wt, lambda a, b: X.s3_model(a, b, drop=(2, 0)))
    err = np.abs(got - want).max() / np.abs(want).max()
    assert 0 < err < 2e-5, err
