"""nn.SyncBatchNorm networks without a GPU: construction and the state_dict surface against the reference's BatchNorm fixtures (a
SyncBatchNorm network IS a BatchNorm2d network until the data-parallel path is on), checkpoint round trips between the two kinds, the
refusals, and the argument checks of the split-form entry points (moments -> coefficients / backward apply)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests.golden_util import GOLDEN_DIR, probe

NAMES = ['bn_a', 'bn_b', 'bn_c', 'bn_w_cfg2']
PG_EINVAL, PG_EWORKSPACE = -1, -2


def _gold(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
    cfg = {k: (v == 'True' if v in ('True', 'False') else (int(v) if v.isdigit() else v)) for k, v in zip(z['cfg_keys'], z['cfg_vals'])}
    return z, cfg


def _modules(cfg, seed=1234, norm_layer=nn.SyncBatchNorm):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(cfg['in_nc'], cfg['out_nc'], cfg['nf'], norm_layer=norm_layer, use_dropout=False, activation=cfg['activation'],
                final_act=cfg['final_act'])
    d = pg.Discriminator(cfg['in_nc'] + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=cfg['norm'], norm_layer=norm_layer)
    return g, d


@pytest.mark.parametrize('name', NAMES)
def test_syncbatchnorm_state_dict_equals_the_reference_fixture(name):
    """Keys, order, shapes, dtypes and initial values of a BatchNorm2d network (tests/test_batchnorm_cpu.py's check)."""
    z, cfg = _gold(name)
    g, d = _modules(cfg, int(z['meta'][0]))
    assert g.engine.has_bn and g.engine.sync_bn and d.engine.sync_bn == bool(cfg['norm'])
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


def test_checkpoints_round_trip_between_batchnorm_and_syncbatchnorm(tmp_path):
    _, cfg = _gold('bn_b')
    gen = torch.Generator().manual_seed(3)
    for src_kind, dst_kind in ((nn.BatchNorm2d, nn.SyncBatchNorm), (nn.SyncBatchNorm, nn.BatchNorm2d)):
        for which in (0, 1):
            src = _modules(cfg, 7, src_kind)[which]
            sd = {k: v.clone() for k, v in src.state_dict().items()}
            for k in sd:
                if 'running' in k:
                    sd[k] = torch.rand(sd[k].shape, generator=gen) + 0.1
                elif 'num_batches_tracked' in k:
                    sd[k] = torch.tensor(17, dtype=torch.int64)
            path = str(tmp_path / f'{src_kind.__name__}_{which}.pth')
            torch.save(sd, path)
            dst = _modules(cfg, 5, dst_kind)[which]
            dst.load_state_dict(torch.load(path))
            back = dst.state_dict()
            assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) and back[k].dtype == sd[k].dtype for k in sd)
            assert dst.engine.nparams == src.engine.nparams and dst.engine.sync_bn == (dst_kind is nn.SyncBatchNorm)


def test_syncbatchnorm_refusals():
    import patchgan_amd as pg
    for bad in (functools.partial(nn.SyncBatchNorm, momentum=0.2), functools.partial(nn.SyncBatchNorm, eps=1e-3),
                functools.partial(nn.SyncBatchNorm, affine=False)):
        with pytest.raises(NotImplementedError, match='InstanceNorm2d or nn.BatchNorm2d'):
            pg.UNet(3, 1, 4, norm_layer=bad)
        with pytest.raises(NotImplementedError, match='InstanceNorm2d or nn.BatchNorm2d'):
            pg.Discriminator(4, 4, norm=True, norm_layer=bad)
    d = pg.Discriminator(4, 4, norm=False, norm_layer=nn.SyncBatchNorm)          # (no norm: the argument is not used)
    assert not d.engine.has_bn and not d.engine.sync_bn
    with pytest.raises(NotImplementedError, match='bf16'):
        pg.UNet(3, 1, 4, norm_layer=nn.SyncBatchNorm).set_precision('bf16')
    with pytest.raises(NotImplementedError, match='bf16'):
        pg.Discriminator(4, 4, norm=True, norm_layer=nn.SyncBatchNorm).set_precision('bf16')
    assert not pg.UNet(3, 1, 4, norm_layer=nn.BatchNorm2d).engine.sync_bn       # BatchNorm2d: never synchronised


def test_no_group_means_no_dist_in_the_bn_run():
    """Without a process group a SyncBatchNorm network's passes carry no Dist: they run the BatchNorm2d code."""
    import patchgan_amd as pg
    g = pg.UNet(3, 1, 4, norm_layer=nn.SyncBatchNorm)
    assert g.bn_run().dist is None
    g.eval()
    assert g.bn_run().dist is None and not g.bn_run().train


def test_split_entry_points_reject_bad_arguments_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(4096)          # a non-null pointer that no refused call may touch
    N, HW, C = 4, 64, 32
    full = int(lib.pg_batchnorm_workspace_bytes(N, HW, C, 1))
    assert full >= 256
    # ---- forward moments
    fwd = lambda **k: lib.pg_batchnorm_moments_fwd(k.get('y', P), k.get('ld', C), k.get('part'), k.get('chunks', 0), k.get('mom', P),
                                                   k.get('N', N), HW, C, k.get('nseg', 1), k.get('ws', P), k.get('wsb', full), None)
    assert fwd(y=None) == PG_EINVAL and fwd(mom=None) == PG_EINVAL and fwd(ld=C - 1) == PG_EINVAL
    assert fwd(N=3, nseg=2) == PG_EINVAL and fwd(nseg=3) == PG_EINVAL and fwd(N=0) == PG_EINVAL
    assert fwd(y=None, part=P, chunks=0) == PG_EINVAL                       # partial sums without a chunk count
    assert fwd(wsb=full - 256) == PG_EWORKSPACE and fwd(ws=None) == PG_EWORKSPACE
    # ---- coefficients
    coef = lambda **k: lib.pg_batchnorm_coef_from_moments(k.get('mom', P), k.get('count', 8.0), k.get('w', P), k.get('b', P), 1e-5,
                                                          k.get('coef', P), None, k.get('C', C), k.get('nseg', 1), None)
    assert coef(mom=None) == PG_EINVAL and coef(w=None) == PG_EINVAL and coef(b=None) == PG_EINVAL and coef(coef=None) == PG_EINVAL
    assert coef(C=0) == PG_EINVAL and coef(nseg=3) == PG_EINVAL
    assert coef(count=1.0) == PG_EINVAL and coef(count=0.0) == PG_EINVAL and coef(count=float('nan')) == PG_EINVAL   # one value per channel
    # ---- backward moments
    bm = lambda **k: lib.pg_batchnorm_moments_bwd(k.get('g1', P), k.get('ld_g1', C), k.get('g2'), k.get('ld_g2', 0), k.get('y', P), C,
                                                  k.get('coef', P), k.get('mom', P), k.get('dw'), k.get('db'), k.get('N', N), HW, C,
                                                  k.get('nseg', 1), k.get('act', 0), k.get('p', 0.0), 0, k.get('ws', P),
                                                  k.get('wsb', full), None)
    assert bm(g1=None) == PG_EINVAL and bm(y=None) == PG_EINVAL and bm(coef=None) == PG_EINVAL and bm(mom=None) == PG_EINVAL
    assert bm(ld_g1=C - 1) == PG_EINVAL and bm(g2=P, ld_g2=C - 1) == PG_EINVAL and bm(dw=P) == PG_EINVAL and bm(db=P) == PG_EINVAL
    assert bm(act=9) == PG_EINVAL and bm(p=1.0) == PG_EINVAL and bm(N=3, nseg=2) == PG_EINVAL
    assert bm(wsb=full - 256) == PG_EWORKSPACE and bm(ws=None) == PG_EWORKSPACE
    # ---- backward apply
    ba = lambda **k: lib.pg_batchnorm_bwd_apply(k.get('g1', P), C, k.get('g2'), k.get('ld_g2', 0), k.get('y', P), C, k.get('coef', P),
                                                k.get('mom', P), k.get('count', 8.0), k.get('dy', P), k.get('ld_dy', C), N, HW, C,
                                                k.get('nseg', 1), k.get('act', 0), k.get('p', 0.0), 0, k.get('ws', P), k.get('wsb', full),
                                                None)
    assert ba(g1=None) == PG_EINVAL and ba(y=None) == PG_EINVAL and ba(coef=None) == PG_EINVAL and ba(mom=None) == PG_EINVAL
    assert ba(dy=None) == PG_EINVAL and ba(ld_dy=C - 1) == PG_EINVAL and ba(g2=P, ld_g2=3) == PG_EINVAL
    assert ba(count=1.0) == PG_EINVAL and ba(act=-1) == PG_EINVAL and ba(p=-0.1) == PG_EINVAL and ba(nseg=3) == PG_EINVAL
    assert ba(wsb=full - 256) == PG_EWORKSPACE and ba(ws=None) == PG_EWORKSPACE
