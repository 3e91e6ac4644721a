"""The yardstick of tests/test_wino1_gpu.py, shown without a GPU: the transform tables of tests/wino1_util.py are those of
conv_wino.hip; run in float64 each model IS the convolution (tables, window origins, tap flip, ragged edges); and the statistic
discriminates -- on a 2048-tile, 64-channel case a GEMM damaged in any of six ways fails the bound against the undamaged fp32
model, while the undamaged sums taken in a shuffled order pass."""
import os
import random

import numpy as np
import pytest
import torch

from tests import exact_util as X
from tests import wino1_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tiny ragged shapes (N, Hb, Wb, Ca, Cb, 1): odd and even extents, one / two leftover rows and columns for both tile edges
TINY = [(2, 7, 8, 5, 3, 1), (1, 9, 6, 2, 4, 1), (2, 5, 11, 3, 2, 1), (1, 8, 8, 1, 1, 1)]
SENS_GEOM = (2, 64, 65, 64, 64, 1)      # forward: 63 x 64 outputs = 32 x 32 F(2x2,4x4) tiles per sample (last tile row ragged), 2048 tiles


def test_table_literals_are_the_kernels():
    src = X.source_tables(os.path.join(ROOT, 'patchgan_amd', 'csrc', 'conv_wino.hip'), W.TABLES)
    assert set(src) == {'c_BT', 'c_G', 'c_AT24', 'c_BT6', 'c_G34', 'c_AT34', 'c_G2', 'c_A4T', 'c_G43', 'c_A4T6'}
    for name, t in W.TABLES.items():
        assert src[name].shape == t.shape and np.array_equal(src[name], t.astype(np.float32)), (name, src[name], t)
    # ... and the extended parser still reads the dyadic tables of the polyphase paths
    dy = X.source_tables(os.path.join(ROOT, 'patchgan_amd', 'csrc', 'conv_wino.hip'))
    assert all(np.array_equal(dy[k], v) for k, v in X.TABLES.items())
    # the tables these kernels are kept out of the exact class for
    assert not set(np.abs(W.c_G).ravel().tolist()) <= {0.0, 0.5, 1.0}


@pytest.mark.parametrize('mo', [2, 3])
@pytest.mark.parametrize('geom', TINY, ids=lambda g: 'x'.join(map(str, g)))
def test_float64_models_are_the_convolution(geom, mo):
    ops = W.normal_operands(geom)
    for op, model, x, bias in ((0, W.wino1_fwd_model, ops.big, ops.bias_a), (1, W.wino1_dgrad_model, ops.small, ops.bias_b)):
        for act in ('none', 'leakyrelu'):
            ref, S = W.ref_and_scale(ops, op, act)
            got = model(x, ops.Wt, mo, torch.float64, bias, act)
            assert got.dtype == torch.float64 and got.shape == ref.shape
            assert float(((got - ref).abs() / S).max()) < 1e-12, (geom, mo, op, act)
    ref, S = W.ref_and_scale(ops, 2)
    got = W.wino1_wgrad_model(ops.big, ops.small, mo, torch.float64)        # (mo serves as the dy tile edge r)
    assert got.shape == ref.shape and float(((got - ref).abs() / S).max()) < 1e-12, (geom, mo)
    # the chunked GEMM of the sensitivity tests is the same sum
    got = W.wino1_fwd_model(ops.big, ops.Wt, mo, torch.float64, gemm=lambda A, B: W.chunk_gemm(A, B, 2, order=[1, 0] if geom[4] > 2 else None))
    ref, S = W.ref_and_scale(ops, 0, bias=False)
    assert float(((got - ref).abs() / S).max()) < 1e-12


def test_planner_rules_mirrored_by_the_util():
    """The dy tile edge the library reports through its executed-FLOP count is wgrad_r's; the tile edge read off a forward symbol is the
    one the library plans (host-side queries, no GPU)."""
    from patchgan_amd import engine as E, _lib as L
    for geom in [(2, 66, 65, 64, 64, 1), (4, 47, 48, 64, 64, 1), (4, 46, 48, 64, 64, 1), (2, 66, 65, 128, 128, 1)]:
        N, Hb, Wb, Ca, Cb, s = geom
        Hs, Ws = X.dims(geom)
        r = W.wgrad_r(N, Hs, Ws)
        op = E.ConvOp(*geom, L.ALGO_AUTO)
        assert op.describe(2)[0].startswith('k_wino_wgrad_gemm'), geom
        assert op.kernel_flops(2) == 2.0 * (r + 3) ** 2 * N * W.tiles(Hs, r) * W.tiles(Ws, r) * Ca * Cb, (geom, r)
        for bits, mo in ((L.TUNE_WINO1_F2, 2), (L.TUNE_WINO1_F3, 3)):
            o = E.ConvOp(*geom, L.ALGO_AUTO | bits)
            assert W.fwd_tile_edge(o.describe(0)[0]) == mo
            assert o.kernel_flops(0) == 2.0 * (mo + 3) ** 2 * N * W.tiles(Hs, mo) * W.tiles(Ws, mo) * Ca * Cb
    assert [W.fwd_slices(2, 65, 64, c, 64) for c in (64, 128, 256, 192)] == [1, 2, 4, 1]


def test_gpu_case_lists_plan_onto_every_family():
    """The static half of the GPU file's coverage guard, from the planner's host-side answers."""
    from tests import test_wino1_gpu as G
    plan = G.check_plan()
    print({k: len(v) for k, v in sorted(plan.items())})
    print('fuzz:', G._fuzz_geoms())


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
class _Sens:
    """Operands, float64 reference and the undamaged fp32 model of the sensitivity case (computed once)."""
    _it = None

    @classmethod
    def get(cls):
        if cls._it is None:
            cls._it = cls()
        return cls._it

    def __init__(self):
        self.ops = W.normal_operands(SENS_GEOM)
        self.ref, self.S = W.ref_and_scale(self.ops, 0, 'leakyrelu')
        self.model = self.stat(self.run())

    def run(self, **kw):
        o = self.ops
        return W.wino1_fwd_model(o.big, o.Wt, 2, torch.float32, o.bias_a, 'leakyrelu', **kw)

    def stat(self, got):
        return W.Stat(got, self.ref, self.S)


def _np_gemm(fa, fb):
    """matmul_gemm on operands passed through NumPy functions (the bf16 helpers of exact_util)."""
    t = lambda f, a: torch.from_numpy(np.ascontiguousarray(f(a.numpy())))
    return lambda A, B: W.matmul_gemm(t(fa, A), t(fb, B))


def _two_pieces_without_02(A, B):
    """One operand without its third bf16 piece, and the product (0, 2) dropped as well: (a1 + a2) b - a1 b3."""
    a1, a2, _ = X.s3_split(A.numpy())
    b3 = X.s3_split(B.numpy())[2]
    t = torch.from_numpy
    return W.matmul_gemm(t(a1 + a2), B) - W.matmul_gemm(t(a1), t(b3))


def _swap_tiles(M, V, U):
    M = M.clone()
    t = 31 * 32 + 5                  # two neighbours in the ragged last tile row of sample 0
    M[:, [t, t + 1]] = M[:, [t + 1, t]]
    return M


def _slab_twice(M, V, U):
    M = M.clone()
    t = 1024 + 31 * 32 + 9           # a ragged tile of sample 1: the second K slice (channels 32 .. 63) once more
    M[:, t] += torch.einsum('pk,pok->po', V[:, t, 32:], U[:, :, 32:])
    return M


DAMAGED = {
    'a transform point loses one 32-wide K chunk': dict(gemm=lambda A, B: W.chunk_gemm(A, B, 32, skip=[(7, 1)])),
    'one operand rounded to bf16': dict(gemm=_np_gemm(X.bf16_rne, lambda b: b)),
    'the other operand rounded to bf16': dict(gemm=_np_gemm(lambda a: a, X.bf16_rne)),
    'third split piece and the (0,2) product lost': dict(gemm=_two_pieces_without_02),
    'two tiles swapped at the ragged edge': dict(damage_m=_swap_tiles),
    'a K-slice slab added twice in one tile': dict(damage_m=_slab_twice),
}


@pytest.mark.parametrize('what', list(DAMAGED))
def test_damaged_gemm_fails_the_bound(what):
    s = _Sens.get()
    k = s.stat(s.run(**DAMAGED[what]))
    print(W.report(what, k, s.model))
    assert not W.within(k, s.model), what


def test_one_wrong_edge_element_fails_the_bound():
    s = _Sens.get()
    got = s.run().clone()
    got[0, 3, 62, 10] = got[0, 3, 62, 11]        # a ragged-edge element replaced by its neighbour
    k = s.stat(got)
    print(W.report('one ragged-edge element replaced by its neighbour', k, s.model))
    assert not W.within(k, s.model)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_another_summation_order_passes(seed):
    """The undamaged sums, K taken in 8-wide chunks in a shuffled order: inside the margins (they are not too tight)."""
    s = _Sens.get()
    order = list(range(8))
    random.Random(seed).shuffle(order)
    k = s.stat(s.run(gemm=lambda A, B: W.chunk_gemm(A, B, 8, order=order)))
    print(W.report(f'chunk order {order}', k, s.model))
    assert W.within(k, s.model), (k, s.model)


def test_probe_sees_what_a_dense_norm_cannot():
    """Step 3 on the model: with the input confined to the last sample's last two rows and columns the quiet tiles return the bias
    exactly, and the touched ones meet the bound; a slab added to a tile of another sample, or a tile decoded into the wrong sample,
    fails the exact comparison."""
    s = _Sens.get()
    o = s.ops
    N, Hb, Wb = SENS_GEOM[:3]
    probe = W.replaced(o, big=W.corner_input(o.big))
    ref, S = W.ref_and_scale(probe, 0)
    quiet = W.quiet_mask(N, Hb, Wb, 1, 2)
    assert bool(quiet[0].all()) and not bool(quiet[-1, -1].any()) and bool(quiet[-1, 0, 0]) and 0 < int((~quiet).sum()) < quiet[-1].numel() // 4
    assert torch.equal(ref[quiet[:, None].expand_as(ref)], o.bias_a.double().view(1, -1, 1, 1).expand_as(ref)[quiet[:, None].expand_as(ref)])
    run = lambda dtype, **kw: W.wino1_fwd_model(probe.big, o.Wt, 2, dtype, o.bias_a, **kw)
    bad, model = W.probe_stats(run(torch.float32), ref, S, o.bias_a, quiet)
    assert bad == 0
    order = [3, 1, 0, 2]
    bad, k = W.probe_stats(run(torch.float32, gemm=lambda A, B: W.chunk_gemm(A, B, 16, order=order)), ref, S, o.bias_a, quiet)
    print(W.report('probe, chunk order shuffled', k, model))
    assert bad == 0 and W.within(k, model)

    def wrong_sample(M, V, U):
        M = M.clone()
        M[:, 31 * 32 + 31] = M[:, 1024 + 31 * 32 + 31]       # sample 1's corner tile lands in sample 0 as well
        return M

    def slab_elsewhere(M, V, U):
        M = M.clone()
        M[:, 1024 + 3 * 32 + 4] += 2.0 ** -20 * M[:, 1024 + 31 * 32 + 30]      # (1e-6 of an output: invisible to a 1e-5 max norm)
        return M

    for dmg in (wrong_sample, slab_elsewhere):
        bad, _ = W.probe_stats(run(torch.float32, damage_m=dmg), ref, S, o.bias_a, quiet)
        assert bad > 0, dmg.__name__
