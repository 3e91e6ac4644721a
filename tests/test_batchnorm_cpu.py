"""nn.BatchNorm2d networks without a GPU: construction, the state_dict surface against the reference's BatchNorm fixtures
(tests/golden/make_golden_bn.py), checkpoint round trips, transfer loads, the refusals and the C ABI's argument checks."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests.golden_util import GOLDEN_DIR, probe

NAMES = ['bn_a', 'bn_b', 'bn_c', 'bn_w_cfg2']


def _gold(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
    cfg = {k: (v == 'True' if v in ('True', 'False') else (int(v) if v.isdigit() else v)) for k, v in zip(z['cfg_keys'], z['cfg_vals'])}
    return z, cfg


def _modules(cfg, seed=1234):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(cfg['in_nc'], cfg['out_nc'], cfg['nf'], norm_layer=nn.BatchNorm2d, use_dropout=False, activation=cfg['activation'],
                final_act=cfg['final_act'])
    d = pg.Discriminator(cfg['in_nc'] + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=cfg['norm'],
                         norm_layer=nn.BatchNorm2d)
    return g, d


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_equals_the_reference_fixture(name):
    """Keys, order, shapes, dtypes and initial values (conv weights under the fixture's seed bit for bit; BatchNorm: weight 1,
    bias 0, running_mean 0, running_var 1, num_batches_tracked 0)."""
    z, cfg = _gold(name)
    g, d = _modules(cfg, int(z['meta'][0]))
    for prefix, net in (('g0/', g), ('d0/', d)):
        sd = net.state_dict()
        assert list(sd) == list(z[prefix + 'keys'])
        assert [','.join(str(s) for s in v.shape) for v in sd.values()] == list(z[prefix + 'shapes'])
        assert [str(v.dtype) for v in sd.values()] == list(z[prefix + 'dtypes'])
        for k, v in sd.items():
            full = z.get(prefix + 'full/' + k) if (prefix + 'full/' + k) in z.files else None
            if full is not None:
                assert torch.equal(v, torch.from_numpy(full)), k
            else:
                assert np.array_equal(probe(v)[2:], z[prefix + 'probe/' + k][2:]), k
    keys = list(g.state_dict())
    assert len(keys) == 74 and keys[1:6] == ['encoder.0.model.DownNorm0.' + s for s in
                                             ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]
    assert g.state_dict()['decoder.1.model.UpNorm1.num_batches_tracked'].shape == ()


def test_checkpoint_round_trip_with_moved_running_statistics(tmp_path):
    _, cfg = _gold('bn_b')
    g, d = _modules(cfg)
    sd = {k: v.clone() for k, v in d.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    for k in sd:
        if 'running' in k:
            sd[k] = torch.rand(sd[k].shape, generator=gen) + 0.1
        elif 'num_batches_tracked' in k:
            sd[k] = torch.tensor(17, dtype=torch.int64)
    torch.save(sd, str(tmp_path / 'd.pth'))
    _, d2 = _modules(cfg, seed=5)
    d2.load_state_dict(torch.load(str(tmp_path / 'd.pth')))
    back = d2.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # the buffers are module buffers that view the buffer block: buffers() sees them, Adam's parameter buffer does not hold them
    names = [n for n, _ in d2.named_buffers()]
    assert names == [k for k in sd if 'running' in k or 'num_batches' in k]
    flat_storage = d2.flat.untyped_storage().data_ptr()
    assert all(p.untyped_storage().data_ptr() == flat_storage for p in d2.parameters())
    assert all(b.untyped_storage().data_ptr() != flat_storage for b in d2.buffers())


def test_transfer_from_an_instancenorm_checkpoint_leaves_batchnorm_alone():
    import patchgan_amd as pg
    torch.manual_seed(1)
    src = pg.UNet(3, 1, 4)
    g = pg.UNet(3, 1, 4, norm_layer=nn.BatchNorm2d)
    before = {k: v.clone() for k, v in g.state_dict().items()}
    g.load_transfer_data(src.state_dict())
    after = g.state_dict()
    for k, v in after.items():
        if 'Norm' in k:
            assert torch.equal(v, before[k]), k
        else:
            assert torch.equal(v, src.state_dict()[k]), k


def test_refusals():
    import patchgan_amd as pg
    for bad in (nn.LayerNorm, nn.GroupNorm, functools.partial(nn.BatchNorm2d, momentum=0.2)):
        with pytest.raises(NotImplementedError, match='InstanceNorm2d or nn.BatchNorm2d'):
            pg.UNet(3, 1, 4, norm_layer=bad)
        with pytest.raises(NotImplementedError, match='InstanceNorm2d or nn.BatchNorm2d'):
            pg.Discriminator(4, 4, norm=True, norm_layer=bad)
    pg.Discriminator(4, 4, norm=False, norm_layer=nn.LayerNorm)          # (no norm: the argument is not used, as in the reference)
    with pytest.raises(NotImplementedError, match='bf16'):
        pg.UNet(3, 1, 4, norm_layer=nn.BatchNorm2d).set_precision('bf16')
    with pytest.raises(NotImplementedError, match='bf16'):
        pg.Discriminator(4, 4, norm=True, norm_layer=nn.BatchNorm2d).set_precision('bf16')
    pg.UNet(3, 1, 4).set_precision('bf16')                              # InstanceNorm networks: unchanged


def test_instancenorm_layout_is_unchanged():
    """An InstanceNorm network keeps its flat parameter layout and registers no buffers."""
    import patchgan_amd as pg
    from patchgan_amd import engine as E
    g = pg.UNet(3, 1, 64)
    assert g.engine.nparams == E.assign_offsets(E.unet_layers(3, 1, 64, 'tanh', 'softmax', False)[0] +
                                                E.unet_layers(3, 1, 64, 'tanh', 'softmax', False)[1])
    assert list(g.buffers()) == [] and not g.engine.has_bn
    assert len(g.state_dict()) == 14


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    assert lib.pg_batchnorm_workspace_bytes(4, 64, 32, 1) > 0
    assert lib.pg_batchnorm_workspace_bytes(3, 64, 32, 2) == 0                  # N not a multiple of the segments
    assert lib.pg_batchnorm_act_fwd(None, 4, None, 4, None, None, None, None, 2, 4, 4, 1, 0, 1e-5, 0.0, 0, None, 0, None) == -1
    assert lib.pg_batchnorm_stats(None, 4, None, 0, None, None, None, None, 2, 4, 4, 1, 1e-5, None, 0, None) == -1
    assert lib.pg_batchnorm_act_apply(None, 4, None, 4, None, 2, 4, 4, 1, 0, 0.0, 0, None) == -1
    assert lib.pg_batchnorm_eval_coef(None, None, None, None, 4, 1e-5, None, None) == -1
    assert lib.pg_batchnorm_act_bwd(None, 4, None, 0, None, 4, None, None, 4, None, None, 2, 4, 4, 1, 1, 0, 0.0, 0, None, 0,
                                    None) == -1
    assert lib.pg_batchnorm_update_running(0, None, 1, 0.1, None) == -1
    items = (_lib.BnUpdateItem * 1)()
    assert lib.pg_batchnorm_update_running(1, items, 1, 0.1, None) == -1       # null pointers in the item
    # one value per channel in training mode (M = 1) is refused by the kernels' own check too
    assert lib.pg_batchnorm_act_fwd(ctypes.c_void_p(16), 4, ctypes.c_void_p(16), 4, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                    ctypes.c_void_p(16), None, 2, 1, 4, 2, 0, 1e-5, 0.0, 0, None, 0, None) == -1
