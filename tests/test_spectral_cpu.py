"""Spectral normalisation of the discriminator, the parts that need no GPU: the module's torch surface against the fixtures made
from torch.nn.utils.spectral_norm on the reference (tests/golden/sn_a_*.npz, make_golden_sn.py), the YAML key, and the float64
reference / fp32 emulation of tests/spectral_util.py -- which the GPU tests hold the kernels to -- against the fixture, against
torch's autograd, and against the planted mutations its comparator must reject."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from tests import spectral_util as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODULE_FIXTURES = {'sn_a_plain': False, 'sn_a_norm': True}


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def disc(norm, **kw):
    import patchgan_amd as pg
    return pg.Discriminator(5, 8, n_layers=3, norm=norm, spectral_norm=True, **kw)


def state0(z):
    return {k: torch.from_numpy(z['sd0/' + k].copy()) for k in z['keys']}


@pytest.mark.parametrize('name', list(MODULE_FIXTURES))
def test_state_dict_is_torchs_spectral_norm_layout(name):
    z = fixture(name)
    torch.manual_seed(int(z['meta'][0]))
    d = disc(MODULE_FIXTURES[name])
    sd = d.state_dict()
    assert list(sd) == list(z['keys'])
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == list(z['shapes'])
    assert [str(v.dtype) for v in sd.values()] == list(z['dtypes'])
    assert [k for k, _ in d.named_parameters()] == list(z['param_names'])
    assert [k for k, _ in d.named_buffers()] == list(z['buffer_names'])
    assert not any(k.endswith('.weight') and k[:-len('.weight')] + '.weight_orig' in sd for k in sd)
    # the same seed draws the same weights and, after them, the same u and v as the wrapped reference module
    for k, v in sd.items():
        assert torch.equal(v, state0(z)[k]), k
    names = [k for k, _ in d.named_parameters()]
    assert names.index('model.0.bias') < names.index('model.0.weight_orig')


@pytest.mark.parametrize('name', list(MODULE_FIXTURES))
def test_state_dict_loads_and_saves(name):
    z = fixture(name)
    d = disc(MODULE_FIXTURES[name])
    d.load_state_dict(state0(z))
    for k, v in d.state_dict().items():
        assert torch.equal(v, state0(z)[k]), k
    # weight_orig is the view of the flat buffer the kernels read, u / v views of the spectral-norm block
    l = d.engine.layers[1]
    assert torch.equal(S.unpack(d.flat[l.p_off:l.p_off + 16 * l.a * l.b], l.a, l.b), state0(z)[l.key])
    assert torch.equal(d.sn_bufs[l.u_off:l.u_off + l.a], state0(z)[l.key[:-5] + '_u'])
    # what save() writes: a plain dict of contiguous tensors, no _metadata -- it loads into the same key set
    saved = d.state_dict_contiguous()
    assert type(saved) is dict and all(v.is_contiguous() for v in saved.values())
    d2 = disc(MODULE_FIXTURES[name])
    assert d2.load_state_dict(saved).missing_keys == []
    assert torch.equal(d2.flat, d.flat) and torch.equal(d2.sn_bufs, d.sn_bufs)


def test_initial_u_v_have_unit_norm():
    d = disc(True)
    for k, b in d.named_buffers():
        assert k.endswith(('weight_u', 'weight_v'))
        assert abs(float(b.double().norm()) - 1.0) < 1e-6, k


def test_option_is_a_bool_and_off_changes_nothing():
    import patchgan_amd as pg
    from patchgan_amd import engine as E
    for bad in (1, 0, 'true', None):
        with pytest.raises(TypeError, match='spectral_norm'):
            pg.Discriminator(5, 8, spectral_norm=bad)
    torch.manual_seed(5)
    d = pg.Discriminator(5, 8, n_layers=3, norm=True)
    torch.manual_seed(5)
    off = pg.Discriminator(5, 8, n_layers=3, norm=True, spectral_norm=False)
    assert list(d.state_dict()) == list(off.state_dict()) == E.param_keys(off.engine.layers)
    assert list(off.buffers()) == [] and not off.spectral_norm and off.engine.nsn == 0
    assert torch.equal(d.flat, off.flat)
    with pytest.raises(RuntimeError, match='spectral_norm'):
        off.spectral_normalize()
    with pytest.raises(RuntimeError, match='HIP device'):
        disc(False).spectral_normalize()          # (on the CPU: refused, no fallback)


NESTED = """
dataset: {type: X, data: {images: a, masks: b}, train_val_split: [0.8, 0.2]}
model_params:
  generator: {filters: 8, activation: relu}
  discriminator: {filters: 4, n_layers: 3, norm: true%s}
"""
FLAT = """
dataset: {type: X, data: {images: a, masks: b}, train_val_split: [0.8, 0.2]}
model_params: {gen_filts: 8, disc_filts: 4, n_disc_layers: 3, activation: relu%s}
"""


def test_yaml_key_in_both_schemas():
    from patchgan_amd.train import model_cfgs, parse_config, spectral_norm_of
    assert spectral_norm_of() is False and spectral_norm_of(None) is False and spectral_norm_of(True) is True
    assert parse_config(yaml.safe_load(NESTED % ', spectral_norm: true'))[5]['spectral_norm'] is True
    assert parse_config(yaml.safe_load(FLAT % ', disc_spectral_norm: true'))[5]['spectral_norm'] is True
    assert parse_config(yaml.safe_load(FLAT % ', disc_spectral_norm: false'))[5]['spectral_norm'] is False
    assert 'spectral_norm' not in parse_config(yaml.safe_load(NESTED % ''))[5]
    assert 'spectral_norm' not in parse_config(yaml.safe_load(FLAT % ''))[5]
    for text in (NESTED % ', spectral_norm: 1', NESTED % ', spectral_norm: "yes"', FLAT % ', disc_spectral_norm: 3'):
        with pytest.raises(ValueError, match='spectral_norm'):
            parse_config(yaml.safe_load(text))          # (before anything is built)
        with pytest.raises(ValueError, match='spectral_norm'):
            model_cfgs(yaml.safe_load(text)['model_params'])


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from patchgan_amd import _lib as L
    lib = L.load()
    items = (L.SpectralItem * 1)()
    items[0].Cout, items[0].Cin = 8, 5
    need = lib.pg_spectral_workspace_bytes(1, items)
    assert need > 0 and need % 8 == 0
    assert lib.pg_spectral_workspace_bytes(0, items) == 0 and lib.pg_spectral_workspace_bytes(L.SN_MAX_LAYERS + 1, items) == 0
    assert lib.pg_spectral_workspace_bytes(1, None) == 0
    assert lib.pg_spectral_fwd(1, items, None, None, 0, None, 0, None) == -1          # NULL pointers in the item
    assert lib.pg_spectral_bwd(1, items, None, 0, None, 0, None) == -1
    for f in ('W', 'w_hat', 'u', 'v', 'sigma'):
        setattr(items[0], f, 4096)
    assert lib.pg_spectral_fwd(1, items, None, None, 0, None, need, None) == -1       # NULL workspace
    assert lib.pg_spectral_fwd(1, items, None, None, 0, 4096, need - 8, None) == -1   # workspace too small
    assert lib.pg_spectral_fwd(0, items, None, None, 0, 4096, need, None) == -1
    assert lib.pg_spectral_fwd(1, items, 4096, None, 640, 4096, need, None) == -1     # flat without eff
    assert lib.pg_spectral_fwd(1, items, 8192, 16384, 640, 4096, need, None) == -1    # W not inside flat
    items[0].W = 4100
    assert lib.pg_spectral_fwd(1, items, None, None, 0, 4096, need, None) == -1       # misaligned W
    items[0].W, items[0].Cin = 4096, 0
    assert lib.pg_spectral_fwd(1, items, None, None, 0, 4096, 1 << 20, None) == -1
    items[0].Cin, items[0].g_off = 5, 2
    assert lib.pg_spectral_bwd(1, items, 4096, 1 << 20, 4096, need, None) == -1       # g_off not a multiple of 4
    items[0].g_off = 640
    assert lib.pg_spectral_bwd(1, items, 4096, 1000, 4096, need, None) == -1          # the block ends beyond the gradient
    assert ctypes.sizeof(L.SpectralItem) == 64


# ---- the util's reference and emulation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(MODULE_FIXTURES))
def test_reference_and_emulation_agree_with_the_fixture(name):
    """One training-mode forward of torch's hook moved u, v of every layer: the float64 reference reproduces the fixture's float64
    buffers, the emulation (fp64 sums, fp32 stores) the fixture's fp32 buffers to a few eps32 (torch sums in fp32)."""
    z = fixture(name)
    sd = state0(z)
    for k in z['keys']:
        if not k.endswith('weight_orig'):
            continue
        stem = k[:-len('_orig')]
        W, u0, v0 = sd[k], sd[stem + '_u'], sd[stem + '_v']
        ref = S.power_step(W, u0, v0, True)
        emu = S.emulate(W, u0, v0, True)
        for leaf in ('u', 'v'):
            want64, want32 = torch.from_numpy(z[f'buf64/{stem}_{leaf}']), torch.from_numpy(z[f'buf32/{stem}_{leaf}'])
            assert S.rel_dist(ref[leaf], want64) < 1e-12, (k, leaf)
            assert S.rel_dist(emu[leaf], want32) < 64 * S.EPS32, (k, leaf)
        assert all(r <= 1.0 for r in S.stage_ratios(W, u0, v0, emu, True).values())


def test_gradient_formula_is_torchs_autograd():
    """dW = (dW_hat - <dW_hat, W_hat> u v^T) / sigma with u, v constant and sigma differentiated, in float64."""
    for a, b in ((8, 5), (1, 64)):
        W, u0, v0, g = S.layer_inputs(a, b)
        ref = S.power_step(W, u0, v0, True)
        Wd = W.double().requires_grad_(True)
        sigma = (ref['u'] * (Wd.reshape(a, -1) @ ref['v'])).sum()
        ((Wd / sigma) * g.double()).sum().backward()
        dW = S.grad_map(g, ref['w_hat'], ref['u'], ref['v'], ref['sigma'])[0]
        assert S.rel_dist(dW, Wd.grad) < 1e-12
        assert abs(float(sigma.detach()) - float(ref['sigma'])) < 1e-14


@pytest.mark.parametrize('shape', S.KERNEL_SHAPES[:3])
@pytest.mark.parametrize('iterate', [True, False])
def test_emulation_passes_its_own_comparator(shape, iterate):
    W, u0, v0, g = S.layer_inputs(*shape)
    r = S.stage_ratios(W, u0, v0, S.emulate(W, u0, v0, iterate, g), iterate, g)
    assert all(x <= 1.0 for x in r.values()), r


def test_comparator_rejects_the_planted_mutations():
    W, u0, v0, g = S.layer_inputs(40, 24)
    for mut, key in (('dw_no_second_term', 'dW'), ('sigma_old_u', 'sigma'), ('v_packed_order', 'v')):
        r = S.stage_ratios(W, u0, v0, S.emulate(W, u0, v0, True, g, mut=mut), True, g)
        assert r[key] > 100.0, (mut, r)
    # eps omitted: a u orthogonal to every column of Wm (row 0 of W is 1e-20 of noise, u = e_0) leaves t ~ 1e-20, far below eps --
    # v = t / eps is ~1e-8 of a unit vector; without the clamp it IS a unit vector
    Wz = W.clone()
    Wz[0] *= 1e-20
    e0 = torch.zeros(40)
    e0[0] = 1.0
    ok = S.emulate(Wz, e0, v0, True)
    assert float(ok['v'].norm()) < 1e-6 and S.stage_ratios(Wz, e0, v0, ok, True)['v'] <= 1.0
    assert S.stage_ratios(Wz, e0, v0, S.emulate(Wz, e0, v0, True, mut='no_eps'), True)['v'] > 100.0
    # bias block scaled by 1 / sigma: everything outside the weight blocks is a bit-exact copy
    d = disc(True)
    sigmas = [S.emulate(p.detach(), d.state_dict()[k[:-5] + '_u'], d.state_dict()[k[:-5] + '_v'], False)['sigma']
              for k, p in d.named_parameters() if k.endswith('weight_orig')]
    good, bad = S.effective_flat(d.flat, d.engine.layers, sigmas), S.effective_flat(d.flat, d.engine.layers, sigmas, 'bias_scaled')
    outside = torch.ones(d.flat.numel(), dtype=torch.bool)
    for l in d.engine.layers:
        outside[l.p_off:l.p_off + 16 * l.a * l.b] = False
    assert torch.equal(good[outside], d.flat[outside]) and not torch.equal(bad[outside], d.flat[outside])
    assert not torch.equal(good[~outside], d.flat[~outside])
