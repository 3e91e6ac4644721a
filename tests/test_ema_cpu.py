"""The generator's weight average (Trainer.ema_decay) without a GPU: the C ABI of pg_adam_ema_step / pg_adam_ema_step_dev (argument
validation happens before any launch), the trainer's state (creation, views, lifetime), checkpoints and the YAML key."""
import os
import re

import pytest
import torch
import yaml
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pg_adam_ema_step', 'pg_adam_ema_step_dev')


def _nets(norm_layer=nn.InstanceNorm2d, seed=3):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, 1, 4, norm_layer=norm_layer, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    return g, d


def _trainer(tmp_path, decay, **kw):
    import patchgan_amd as pg
    g, d = _nets(**kw)
    t = pg.Trainer(g, d, str(tmp_path))
    t.ema_decay = decay
    return t


# ---------------------------------------------------------------------------------------------- 1. C ABI
def test_new_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # five buffers, n, then the scalars of pg_adam_step / pg_adam_step_dev with the decay in front of the stream
    assert len(_lib.SIGNATURES['pg_adam_ema_step'][1]) == len(_lib.SIGNATURES['pg_adam_step'][1]) + 2
    assert len(_lib.SIGNATURES['pg_adam_ema_step_dev'][1]) == len(_lib.SIGNATURES['pg_adam_step_dev'][1]) + 2


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.999, None)
    tail_dev = (0.9, 0.999, 1e-8, a, 0.999, None)
    assert lib.pg_adam_ema_step(None, None, None, None, None, 10, *tail) == -1
    assert lib.pg_adam_ema_step_dev(None, None, None, None, None, 10, *tail_dev) == -1
    for i in range(5):                                  # each pointer on its own
        ptrs = [a] * 5
        ptrs[i] = None
        assert lib.pg_adam_ema_step(*ptrs, 10, *tail) == -1, i
        assert lib.pg_adam_ema_step_dev(*ptrs, 10, *tail_dev) == -1, i
    assert lib.pg_adam_ema_step_dev(a, a, a, a, a, 10, 0.9, 0.999, 1e-8, None, 0.999, None) == -1      # scalars
    for n in (0, -4):
        assert lib.pg_adam_ema_step(a, a, a, a, a, n, *tail) == -1
        assert lib.pg_adam_ema_step_dev(a, a, a, a, a, n, *tail_dev) == -1
    for decay in (1.0, 1.5, -0.1, float('nan'), float('inf')):
        assert lib.pg_adam_ema_step(a, a, a, a, a, 10, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, decay, None) == -1, decay
        assert lib.pg_adam_ema_step_dev(a, a, a, a, a, 10, 0.9, 0.999, 1e-8, a, decay, None) == -1, decay
    assert lib.pg_adam_ema_step(a, a, a, a, a + 4, 10, *tail) == -1                                    # misaligned ema


# ---------------------------------------------------------------------------------------------- 2. trainer state
@pytest.mark.parametrize('decay', [1.0, -0.1, float('nan'), 'x'], ids=['one', 'negative', 'nan', 'string'])
def test_bad_decay_raises_value_error(tmp_path, decay):
    t = _trainer(tmp_path, decay)
    with pytest.raises(ValueError):
        t.setup_optimizers()
    assert t._ema is None
    # ... and when a step is enqueued: the decay is part of the step's kind
    t2 = _trainer(tmp_path, 0.9)
    t2.setup_optimizers()
    t2.ema_decay = decay
    with pytest.raises(ValueError):
        t2._adam_step('g')
    x = torch.zeros(2, 3, 256, 256)
    with pytest.raises(ValueError):
        t2._kind_key(x, x[:, :1], False, (2, 256, 256, 3, 1), True)


def test_off_by_default(tmp_path):
    import patchgan_amd as pg
    assert pg.Trainer.ema_decay is None
    t = _trainer(tmp_path, None)
    t.setup_optimizers()
    assert t.ema_generator is None and t._ema is None
    with pytest.raises(RuntimeError):
        t.reset_ema()
    # set after setup_optimizers(): it starts with the next one
    t.ema_decay = 0.99
    assert t.ema_generator is None and t._ema_now() is None
    t.setup_optimizers()
    assert t.ema_generator is not None and t._ema_now() == 0.99
    t.ema_decay = None
    assert t.ema_generator is None and t._ema_now() is None


@pytest.mark.parametrize('norm_layer', [nn.InstanceNorm2d, nn.BatchNorm2d], ids=['instancenorm', 'batchnorm'])
def test_state_views_and_lifetime(tmp_path, norm_layer):
    import patchgan_amd as pg
    t = _trainer(tmp_path, 0.999, norm_layer=norm_layer)
    G = t.generator
    if norm_layer is nn.BatchNorm2d:        # running statistics that are not the initial ones
        with torch.no_grad():
            for k, b in G.named_buffers():
                b.copy_(torch.full_like(b, 3) if b.dtype == torch.int64 else torch.rand(b.shape) + 0.5)
    rng = torch.get_rng_state()
    t.setup_optimizers()
    assert torch.equal(torch.get_rng_state(), rng)              # data loaders shuffle from torch's global RNG
    E = t.ema_generator
    assert isinstance(E, pg.UNet) and not E.training and G.training
    assert (E.engine.input_nc, E.engine.output_nc, E.engine.nf, E.engine.activation, E.engine.final_act, E.engine.use_dropout,
            E.engine.has_bn, E.engine.sync_bn, E.engine.algo, E.engine.act_bf) == (
            G.engine.input_nc, G.engine.output_nc, G.engine.nf, G.engine.activation, G.engine.final_act, G.engine.use_dropout,
            G.engine.has_bn, G.engine.sync_bn, G.engine.algo, G.engine.act_bf)
    gs, es = G.state_dict(), E.state_dict()
    assert list(gs) == list(es)
    for k in gs:
        assert es[k].shape == gs[k].shape and es[k].dtype == gs[k].dtype and torch.equal(es[k], gs[k]), k
    if norm_layer is nn.BatchNorm2d:
        assert any(k.endswith('running_var') for k in es)
        for (k, a), (_, b) in zip(G.named_buffers(), E.named_buffers()):
            assert a.data_ptr() == b.data_ptr(), k            # the live generator's own tensors: always current
    assert t._ema.data_ptr() != G.flat.data_ptr() and t._ema.shape == G.flat.shape and t._ema.dtype == torch.float32
    assert E.flat is t._ema
    # the kernel's in-place update of the flat buffer is what state_dict() sees
    with torch.no_grad():
        t._ema.add_(1.0)
    k0 = 'encoder.0.model.DownConv0.weight'
    assert torch.equal(E.state_dict()[k0], gs[k0] + 1.0) and torch.equal(G.state_dict()[k0], gs[k0])
    # not optimizer state: a second setup_optimizers() keeps it
    before, ptr, net = t._ema.clone(), t._ema.data_ptr(), E
    t.setup_optimizers(5e-4, 5e-4)
    assert t._ema.data_ptr() == ptr and torch.equal(t._ema, before) and t.ema_generator is net
    # reset_ema(): back to the live weights
    with torch.no_grad():
        G.flat.mul_(0.5)
    t.reset_ema()
    assert t._ema.data_ptr() == ptr and torch.equal(t._ema, G.flat) and not torch.equal(t._ema, before)
    assert t._graph_ptrs()[-1] == ptr


# ---------------------------------------------------------------------------------------------- 3. checkpoints
def test_checkpoints(tmp_path, capsys):
    import patchgan_amd as pg
    folder = tmp_path / 'ck'
    t = _trainer(folder, 0.9)
    t.setup_optimizers()
    with torch.no_grad():
        t._ema.mul_(1.25)           # an average that differs from the live weights
    ema_saved, g_saved = t._ema.clone(), t.generator.flat.clone()
    t.save(3)
    names = ['discriminator_ep_003.pth', 'generator_ema_ep_003.pth', 'generator_ep_003.pth']
    assert sorted(os.listdir(folder)) == names
    sd, gsd = torch.load(folder / names[1]), torch.load(folder / names[2])
    assert list(sd) == list(gsd) and all(sd[k].shape == gsd[k].shape and sd[k].is_contiguous() for k in sd)
    fresh = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(fresh.flat, ema_saved)

    # resume into different networks
    t2 = _trainer(folder, 0.9, seed=11)
    assert not torch.equal(t2.generator.flat, g_saved)
    t2.load_last_checkpoint()
    assert t2.start == 4
    assert torch.equal(t2.generator.flat, g_saved) and torch.equal(t2._ema, ema_saved)
    assert torch.equal(t2.ema_generator.state_dict()['decoder.6.model.UpConv6.weight'], sd['decoder.6.model.UpConv6.weight'])

    # without the ema file: the same epoch, the average restarts from the loaded generator
    os.remove(folder / names[1])
    t3 = _trainer(folder, 0.9, seed=12)
    t3.setup_optimizers()
    capsys.readouterr()
    t3.load_last_checkpoint()
    assert t3.start == 4
    assert torch.equal(t3.generator.flat, g_saved) and torch.equal(t3._ema, g_saved)
    assert 'restarts from the loaded generator' in capsys.readouterr().out

    # feature off: two files, as before
    off = tmp_path / 'off'
    t4 = _trainer(off, None)
    t4.setup_optimizers()
    t4.save(3)
    assert sorted(os.listdir(off)) == ['discriminator_ep_003.pth', 'generator_ep_003.pth']


# ---------------------------------------------------------------------------------------------- 4. YAML
TRAIN_YAML = """
train_params:
  loss_type: weighted_bce
  seg_alpha: 100
  gen_learning_rate: 1.e-3
  disc_learning_rate: 1.e-3
  ema_decay: 0.999
"""


def test_yaml_key_reaches_the_trainer(tmp_path):
    from patchgan_amd.train import apply_train_params
    t = _trainer(tmp_path, None)
    cfg = yaml.safe_load(TRAIN_YAML)
    apply_train_params(t, cfg['train_params'])
    assert t.ema_decay == 0.999 and t.loss_type == 'weighted_bce' and t.seg_alpha == 100
    t.setup_optimizers()
    assert t.ema_generator is not None
    del cfg['train_params']['ema_decay']                    # absent = off
    t = _trainer(tmp_path, 0.5)
    apply_train_params(t, cfg['train_params'])
    assert t.ema_decay is None
