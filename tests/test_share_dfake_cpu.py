"""pg_conv_batch_halves_same: the planner's answer to "do two N-sample calls compute what the 2N-sample call computes?" -- the gate of
the Trainer's shared D(fake) pass.  Planner queries only: no GPU."""
import pytest


def _disc(cfg):
    from patchgan_amd import engine as E
    from tests import bench_layers as BL
    c = BL.CONFIGS[cfg]
    return E.DiscriminatorEngine(3 + c['out_nc'], c['ndf'], c['n_layers'], False), c['batch'], c['size']


@pytest.mark.parametrize('cfg', ['cfg2', 'cfg4'])
def test_every_discriminator_forward_layer_of_the_benchmark_configurations_shares(cfg):
    """Same symbol and split 1 at N and 2N for every D forward call of the committed kernel plan, a kept V in both or in neither."""
    from tests import bench_layers as BL
    de, B, S = _disc(cfg)
    plan = BL.committed_plan()
    for li, (h, w) in enumerate(zip(de.ops(B, S, S), de.ops(2 * B, S, S))):
        assert [h.describe(0)[0]] == plan[f'{cfg}-fp32-d{li}/N-b2s-fwd'] and h.describe(0)[1] == 1, (li, h.describe(0))
        assert [w.describe(0)[0]] == plan.get(f'{cfg}-fp32-d{li}/2N-b2s-fwd', plan[f'{cfg}-fp32-d{li}/N-b2s-fwd']) and w.describe(0)[1] == 1
        assert bool(h.v_bytes()) == bool(w.v_bytes())
        assert h.halves_same(w), (cfg, li, h.describe(0), w.describe(0))
    assert de.halves_ok(B, S, S)


def test_the_predicate_is_false_where_the_plans_differ():
    """Small maps: the implicit GEMM splits K by the batch, tile shapes follow the row count, and the polyphase path starts at 64
    tiles.  Wherever symbol or split differ between N and 2N -- or either call splits K -- the answer is no."""
    from patchgan_amd import engine as E, _lib as L
    differ = split = 0
    for algo in (L.ALGO_AUTO, L.ALGO_AUTO | L.TUNE_WINO2_ALL):
        for N in (1, 2, 3, 4, 8):
            for S in (8, 16, 20, 32, 72):
                h, w = E.ConvOp(N, S, S, 128, 64, 2, algo), E.ConvOp(2 * N, S, S, 128, 64, 2, algo)
                if h.describe(0) != w.describe(0):
                    differ += 1
                    assert not h.halves_same(w), (N, S, h.describe(0), w.describe(0))
                elif h.describe(0)[1] != 1:
                    split += 1
                    assert not h.halves_same(w), (N, S, h.describe(0))
    assert differ > 0 and split > 0
    # the two shapes the kernel tests could not use: under the polyphase path's 64-tile minimum at N, and 64-row against 128-row tiles
    W2 = L.ALGO_AUTO | L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL
    for N, S in ((3, 20), (4, 72)):
        h, w = E.ConvOp(N, S, S, 64, 64, 2, W2), E.ConvOp(2 * N, S, S, 64, 64, 2, W2)
        assert h.describe(0)[0] != w.describe(0)[0] and not h.halves_same(w)
    # a trainer-sized instance: ndf = 64 at batch 2 keeps three passes (tests/test_share_dfake_gpu.py runs it)
    assert not E.DiscriminatorEngine(4, 64, 3, False).halves_ok(2, 256, 256)


def test_networks_outside_the_scope_keep_three_passes():
    from patchgan_amd import engine as E, _lib as L
    assert not E.DiscriminatorEngine(4, 64, 3, True).halves_ok(16, 256, 256)                          # InstanceNorm
    assert not E.DiscriminatorEngine(4, 64, 3, True, norm_kind='batch').halves_ok(16, 256, 256)      # BatchNorm
    assert not E.DiscriminatorEngine(4, 64, 3, False, algo=L.ALGO_BF16).halves_ok(16, 256, 256)      # bf16 networks
