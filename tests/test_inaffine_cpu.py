"""Affine InstanceNorm (functools.partial(nn.InstanceNorm2d, affine=True)) without a GPU: the public surface (norm_kind_of, state_dict
against the reference's fixtures, init, checkpoints, transfer, the EMA twin, the YAML key), the C ABI's argument checks, and the
yardstick of tests/test_inaffine_gpu.py -- the float64 references of tests/inaffine_util.py against float64 torch autograd, the
comparator accepting the plain fp32 evaluation and rejecting every seeded mutation on every case, and each case reaching the kernel
path it is meant for (the plan mirror of tests/normact_util.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests import inaffine_util as A
from tests import normact_util as U
from tests.golden_util import GOLDEN_DIR, probe

AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)
NAMES = ['ina_a', 'ina_b']
PG_EINVAL = -1


def _gold(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
    cfg = {k: (v == 'True' if v in ('True', 'False') else (int(v) if v.isdigit() else v)) for k, v in zip(z['cfg_keys'], z['cfg_vals'])}
    return z, cfg


def _modules(cfg, seed=1234, norm_layer=AFFINE):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(cfg['in_nc'], cfg['out_nc'], cfg['nf'], norm_layer=norm_layer, use_dropout=False, activation=cfg['activation'],
                final_act=cfg['final_act'])
    d = pg.Discriminator(cfg['in_nc'] + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=cfg['norm'], norm_layer=norm_layer)
    return g, d


# ---- public surface -------------------------------------------------------------------------------------------------------------------

def test_norm_kind_of_recognition_and_refusals():
    from patchgan_amd.engine import norm_kind_of
    P = functools.partial
    assert norm_kind_of(P(nn.InstanceNorm2d, affine=True), 'x') == 'instance_affine'
    assert norm_kind_of(P(nn.InstanceNorm2d, affine=True, eps=1e-5, momentum=0.1, track_running_stats=False), 'x') == 'instance_affine'
    assert norm_kind_of(P(nn.InstanceNorm2d, affine=False), 'x') == 'instance'
    assert norm_kind_of(P(nn.InstanceNorm2d), 'x') == 'instance'
    assert norm_kind_of(P(nn.InstanceNorm2d, eps=1e-5), 'x') == 'instance'
    assert norm_kind_of(nn.InstanceNorm2d, 'x') == 'instance' and norm_kind_of(nn.BatchNorm2d, 'x') == 'batch'
    for bad in (P(nn.InstanceNorm2d, affine=True, track_running_stats=True), P(nn.InstanceNorm2d, affine=True, eps=1e-3),
                P(nn.InstanceNorm2d, 1e-5, affine=True), P(nn.InstanceNorm2d, affine=True, momentum=0.2), P(nn.InstanceNorm2d, affine=1),
                P(nn.InstanceNorm2d, affine=True, device='cpu'), P(nn.BatchNorm2d, momentum=0.2), P(nn.BatchNorm2d), nn.GroupNorm,
                nn.LayerNorm):
        with pytest.raises(NotImplementedError, match='InstanceNorm2d or nn.BatchNorm2d'):
            norm_kind_of(bad, 'x')


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_equals_the_reference_fixture(name):
    """Keys, order, shapes and dtypes are the reference's; the conv weights are the fixture's bit for bit (its seed), gamma / beta
    -- which the fixture overwrote -- start at 1 / 0; no buffers."""
    z, cfg = _gold(name)
    g, d = _modules(cfg, int(z['meta'][0]))
    for prefix, net in (('g0/', g), ('d0/', d)):
        sd = net.state_dict()
        assert list(sd) == list(z[prefix + 'keys'])
        assert [','.join(str(s) for s in v.shape) for v in sd.values()] == list(z[prefix + 'shapes'])
        assert [str(v.dtype) for v in sd.values()] == list(z[prefix + 'dtypes'])
        assert list(net.buffers()) == [] and not net.engine.has_bn
        normkeys = {l.norm_key + s for l in net.engine.layers if l.norm_params for s in ('.weight', '.bias')}
        assert len(normkeys) == (24 if net is g else (2 * cfg['n_layers'] if cfg['norm'] else 0))
        for k, v in sd.items():
            if k in normkeys:
                assert z[prefix + 'full/' + k].min() != z[prefix + 'full/' + k].max()         # (the fixture's overwritten values, in full)
                assert torch.equal(v, torch.ones_like(v) if k.endswith('weight') else torch.zeros_like(v)), k
            elif (prefix + 'full/' + k) in z.files:
                assert torch.equal(v, torch.from_numpy(z[prefix + 'full/' + k])), k
            else:
                assert np.array_equal(probe(v)[2:], z[prefix + 'probe/' + k][2:]), k
    keys = list(g.state_dict())
    assert len(keys) == 14 + 2 * 12 and keys[1:3] == ['encoder.0.model.DownNorm0.weight', 'encoder.0.model.DownNorm0.bias']
    assert 'decoder.5.model.UpNorm5.bias' in keys and not any('UpNorm6' in k for k in keys)


def test_conv_weights_equal_the_plain_network_of_the_same_seed_and_the_plain_layout_is_unchanged():
    _, cfg = _gold('ina_b')
    g, d = _modules(cfg)
    gp, dp = _modules(cfg, norm_layer=nn.InstanceNorm2d)
    for net, plain in ((g, gp), (d, dp)):
        sd, sp = net.state_dict(), plain.state_dict()
        assert [k for k in sd if k in sp] == list(sp)
        assert all(torch.equal(sd[k], sp[k]) for k in sp)
        extra = [k for k in sd if k not in sp]
        assert extra and all(torch.equal(sd[k], torch.ones_like(sd[k]) if k.endswith('weight') else torch.zeros_like(sd[k])) for k in extra)
        flat = net.flat.untyped_storage().data_ptr()
        assert all(p.untyped_storage().data_ptr() == flat for p in net.parameters())       # views of the flat buffer
        assert all(l.g_off % 4 == 0 and l.be_off % 4 == 0 for l in net.engine.layers if l.norm)
    # the plain layout: no norm parameters anywhere, the offsets of the conv blocks back to back
    from patchgan_amd import engine as E
    assert all(l.g_off == l.be_off == -1 for l in gp.engine.layers + dp.engine.layers)
    enc, dec = E.unet_layers(3, 3, 4, 'tanh', 'softmax', False)
    assert gp.engine.nparams == E.assign_offsets(enc + dec) == sum(16 * l.a * l.b for l in enc + dec)
    assert g.engine.nparams == gp.engine.nparams + sum(2 * ((l.cout + 3) // 4 * 4) for l in g.engine.layers if l.norm)
    assert g.engine.norm_kind == 'instance_affine' and gp.engine.norm_kind == 'instance'


def test_checkpoint_round_trip(tmp_path):
    _, cfg = _gold('ina_b')
    g, d = _modules(cfg)
    gen = torch.Generator().manual_seed(3)
    for net, fn in ((g, 'g.pth'), (d, 'd.pth')):
        sd = {k: torch.rand(v.shape, generator=gen) - 0.5 for k, v in net.state_dict().items()}
        torch.save(sd, str(tmp_path / fn))
        other = _modules(cfg, seed=5)[0 if net is g else 1]
        other.load_state_dict(torch.load(str(tmp_path / fn)))
        back = other.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_transfer_from_a_plain_checkpoint_leaves_gamma_and_beta_alone():
    import patchgan_amd as pg
    torch.manual_seed(1)
    src = pg.UNet(3, 1, 4)
    g = pg.UNet(3, 1, 4, norm_layer=AFFINE)
    with torch.no_grad():
        for k, v in g.state_dict().items():
            if 'Norm' in k:
                v.copy_(torch.rand(v.shape) + 0.5)
    before = {k: v.clone() for k, v in g.state_dict().items()}
    g.load_transfer_data(src.state_dict())
    for k, v in g.state_dict().items():
        assert torch.equal(v, before[k] if 'Norm' in k else src.state_dict()[k]), k


def test_ema_twin_exposes_the_same_keys():
    import patchgan_amd as pg
    g = pg.UNet(3, 1, 4, norm_layer=AFFINE)
    t = g.twin(g.flat.clone())
    assert t.engine.norm_kind == 'instance_affine' and not t.engine.has_bn
    assert list(t.state_dict()) == list(g.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(t.state_dict().values(), g.state_dict().values()))


def test_nothing_refused_for_batchnorm_is_refused_here():
    import patchgan_amd as pg
    g = pg.UNet(3, 1, 32, norm_layer=AFFINE).set_precision('bf16')
    d = pg.Discriminator(4, 32, norm=True, norm_layer=AFFINE).set_precision('bf16')
    assert g.engine.act_bf and d.engine.act_bf and g.bn_run() is None and d.bn_run() is None


# ---- YAML -----------------------------------------------------------------------------------------------------------------------------

NESTED = """
dataset: {type: X, data: {images: a, masks: b}, train_val_split: [0.8, 0.2]}
model_params:
  generator: {filters: 8, activation: relu%s}
  discriminator: {filters: 4, n_layers: 3, norm: true%s}
"""
FLAT = """
dataset: {type: X, data: {images: a, masks: b}, train_val_split: [0.8, 0.2]}
model_params: {gen_filts: 8, disc_filts: 4, n_disc_layers: 3, activation: relu%s}
"""


def test_yaml_norm_layer_key():
    from patchgan_amd.engine import norm_kind_of
    from patchgan_amd.train import NORM_LAYERS, model_cfgs, norm_layer_of, parse_config
    assert list(NORM_LAYERS) == ['instance', 'instance_affine', 'batch', 'sync_batch']
    kinds = {'instance': 'instance', 'instance_affine': 'instance_affine', 'batch': 'batch', 'sync_batch': 'syncbatch'}
    assert all(norm_kind_of(norm_layer_of(k), 'x') == v for k, v in kinds.items())
    assert norm_layer_of() is nn.InstanceNorm2d and norm_layer_of(None) is nn.InstanceNorm2d
    for bad in ('group', 'Instance', '', 3, True):
        with pytest.raises(ValueError, match='norm_layer'):
            norm_layer_of(bad)
    g, d = parse_config(yaml.safe_load(NESTED % (', norm_layer: instance_affine', ', norm_layer: batch')))[4:]
    assert g['norm_layer'] == 'instance_affine' and d['norm_layer'] == 'batch'
    g, d = parse_config(yaml.safe_load(NESTED % ('', '')))[4:]
    assert 'norm_layer' not in g and 'norm_layer' not in d and norm_layer_of(g.get('norm_layer')) is nn.InstanceNorm2d
    g, d = parse_config(yaml.safe_load(FLAT % ', gen_norm_layer: instance_affine, disc_norm_layer: sync_batch'))[4:]
    assert g['norm_layer'] == 'instance_affine' and d['norm_layer'] == 'sync_batch'
    g, d = parse_config(yaml.safe_load(FLAT % ''))[4:]
    assert 'norm_layer' not in g and 'norm_layer' not in d
    for text in (NESTED % (', norm_layer: group', ''), NESTED % ('', ', norm_layer: layer'), FLAT % ', gen_norm_layer: group',
                 FLAT % ', disc_norm_layer: 7'):
        with pytest.raises(ValueError, match='norm_layer'):
            parse_config(yaml.safe_load(text))
        with pytest.raises(ValueError, match='norm_layer'):
            model_cfgs(yaml.safe_load(text)['model_params'])          # (patchgan_infer's route)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------

def test_c_abi_rejects_bad_arguments_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    N, HW, C = 2, 16, 8
    assert lib.pg_instnorm_affine_workspace_bytes(N, HW, C) == A.workspace_bytes(N, HW, C)
    assert lib.pg_instnorm_affine_workspace_bytes(2, 576, 64) == A.workspace_bytes(2, 576, 64)
    assert lib.pg_instnorm_affine_workspace_bytes(0, HW, C) == 0 and lib.pg_instnorm_affine_workspace_bytes(N, HW, 0) == 0
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)          # 16-byte aligned host memory: every call below must return before it would be touched
    assert p % 16 == 0
    q, ws, wsb = p + 4096, p + 8192, 4096

    def fwd(y=p, ld_y=C, out=q, ld_out=C, gamma=p, beta=p, stats=q, N=N, HW=HW, C=C, act=1, p_=0.0, ws=ws, dt=0):
        return lib.pg_instnorm_affine_act_fwd_t(y, ld_y, out, ld_out, gamma, beta, stats, N, HW, C, act, 1e-5, p_, 0, ws, wsb, None, dt)

    def parts(y=p, ld_y=C, out=q, ld_out=C, gamma=p, beta=p, stats=q, part=ws, chunks=2, N=N, HW=HW, C=C, act=1, p_=0.0, dt=0):
        return lib.pg_instnorm_affine_act_fwd_parts_t(y, ld_y, out, ld_out, gamma, beta, stats, part, chunks, N, HW, C, act, 1e-5, p_, 0,
                                                      None, dt)

    def bwd(g1=p, ld_g1=C, g2=None, ld_g2=0, y=p, ld_y=C, gamma=p, beta=p, stats=p, dy=q, ld_dy=C, dgamma=q, dbeta=q, N=N, HW=HW, C=C,
            act=1, p_=0.0, ws=ws, wsb=wsb, dt=0):
        return lib.pg_instnorm_affine_act_bwd_t(g1, ld_g1, g2, ld_g2, y, ld_y, gamma, beta, stats, dy, ld_dy, dgamma, dbeta, N, HW, C, act,
                                                p_, 0, ws, wsb, None, dt)

    for f in (fwd, parts, bwd):
        for kw in (dict(y=None), dict(gamma=None), dict(beta=None), dict(stats=None), dict(gamma=p + 2), dict(beta=p + 1), dict(C=0),
                   dict(C=-4), dict(N=0), dict(HW=0), dict(ld_y=C - 1), dict(act=9), dict(p_=1.0), dict(dt=64), dict(N=70000)):
            assert f(**kw) == PG_EINVAL, (f.__name__, kw)
    for kw in (dict(out=None), dict(ld_out=C - 1)):
        assert fwd(**kw) == PG_EINVAL and parts(**kw) == PG_EINVAL, kw
    assert parts(part=None) == PG_EINVAL and parts(chunks=0) == PG_EINVAL
    for kw in (dict(g1=None), dict(dy=None), dict(ld_g1=C - 1), dict(ld_dy=C - 1), dict(g2=p, ld_g2=C - 1), dict(dgamma=q, dbeta=None),
               dict(dgamma=None, dbeta=q), dict(dgamma=q + 2), dict(dbeta=q + 3), dict(ws=None), dict(wsb=64), dict(ws=ws + 4)):
        assert bwd(**kw) == PG_EINVAL, kw


# ---- the float64 references against torch autograd ---------------------------------------------------------------------------------------

CASES = A.cases()
TORCH_ACT = {'leaky': lambda z: nn.functional.leaky_relu(z, 0.2), 'tanh': torch.tanh}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = [c for c in CASES if c.name == name][0]
    y, g1, g2, gamma, beta, left = A.inputs(case)
    assert left == 0
    return y, g1, g2, gamma, beta


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_float64_reference_is_torch_autograd_through_instancenorm2d(case):
    N, C, H, W = case.shape
    y, g1, g2, gamma, beta = _inputs(case.name)
    seed = U.seed_of(case)
    for act, p, g2on in U.combos(case):
        ref = A.affine_ref(y, g1, g2 if g2on else None, gamma, beta, act, p, seed)
        m = nn.InstanceNorm2d(C, affine=True, eps=U.EPS).double()
        with torch.no_grad():
            m.weight.copy_(gamma)
            m.bias.copy_(beta)
        x = y.view(N, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
        keep = U.mask_t(seed, y.shape, p).view(N, H, W, C).permute(0, 3, 1, 2)
        out = TORCH_ACT[act](m(x)) * keep * U.keep_scale(p)
        g = (g1 + g2 if g2on else g1).view(N, H, W, C).permute(0, 3, 1, 2)
        out.backward(g)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(N, H * W, C)
        scale = lambda t: t.abs().max().clamp_min(1e-30)
        assert (nhwc(out.detach()) - ref['out']).abs().max() <= 1e-12 * scale(ref['out'])
        assert (nhwc(x.grad) - ref['dy']).abs().max() <= 1e-10 * scale(ref['dy'])
        assert (m.weight.grad - ref['dgamma']).abs().max() <= 1e-11 * scale(ref['dgamma'])
        assert (m.bias.grad - ref['dbeta']).abs().max() <= 1e-11 * scale(ref['dbeta'])


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_comparator_accepts_plain_fp32_and_rejects_every_mutation(case):
    y, g1, g2, gamma, beta = _inputs(case.name)
    assert gamma[0] < 0 and gamma[1] == 0 and gamma[2] == 1 and case.shape[0] >= 2
    seed = U.seed_of(case)
    for act, p, g2on in U.combos(case):
        h2 = g2 if g2on else None
        ref = A.affine_ref(y, g1, h2, gamma, beta, act, p, seed)
        plain = A.plain_affine(y, g1, h2, gamma, beta, act, p, seed)
        ok = A.ratios(case, ref, plain, A.stored_result(case, plain))
        assert max(ok.values()) <= 1.0, (act, p, g2on, ok)
        for mut in A.MUTATIONS:
            bad = A.ratios(case, ref, plain, A.stored_result(case, A.plain_affine(y, g1, h2, gamma, beta, act, p, seed, mut=mut)))
            assert max(bad.values()) > 1.0, (mut, act, p, g2on, bad)


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_reaches_its_path(case):
    N, C, H, W = case.shape
    for bwd in (False, True):
        plan = U.norm_plan(case, bwd)
        assert plan['path'] == case.path and (H * W < 512) == (case.path == 'one-wg')
        want_vec = case.vec if not (case.mix == 'y32_out16' and bwd) else 4
        assert plan['vec'] == want_vec, plan
    assert set(U.combos(case)) == {(a, p, g) for a in ('leaky', 'tanh') for p in (0.0, 0.2) for g in (False, True)}


def test_case_table_covers_every_path():
    plans = {c.name: (U.norm_plan(c)['path'], U.norm_plan(c)['vec'], c.mix) for c in CASES}
    assert plans == {'3x8x2x2': ('one-wg', 4, 'fp32'), '2x12x15x15': ('one-wg', 4, 'fp32'), '2x5x15x15': ('one-wg', 1, 'fp32'),
                     '2x64x24x24': ('fixed', 4, 'fp32'), '2x12x24x24': ('flat', 4, 'fp32'), '2x5x24x24': ('flat', 1, 'fp32'),
                     '2x64x24x24-bf16': ('fixed', 8, 'bf16'), '2x64x24x24-y32_out16': ('fixed', 4, 'y32_out16')}
    assert U.norm_plan(CASES[3])['nchunk'] > 1 and U.norm_plan(CASES[1])['groups'] * U.norm_plan(CASES[1])['G'] >= 3
