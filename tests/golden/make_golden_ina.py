#!/usr/bin/env python3
"""Generate the affine-InstanceNorm golden fixtures by IMPORTING THE REFERENCE (build container only), like make_golden_bn.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ina.py [name ...]

Networks built with norm_layer=functools.partial(nn.InstanceNorm2d, affine=True); after construction every norm weight is overwritten
with seeded U(0.5, 1.5) and every norm bias with seeded U(-0.5, 0.5) (at weight 1, bias 0 a weight missing from the backward is nearly
invisible); the overwritten values are stored in full.  Only DATA is written to ``tests/golden/ina_*.npz``, as make_golden_bn.py
stores it: state_dict keys / shapes / dtypes (values in full up to 4096 elements, probes otherwise), forward probes, gradient probes
of every parameter after step 1, the six loss scalars of K steps, state probes after step K, the batch(train=False) losses, and all
of it again in float64 (the reference's own fp32-vs-float64 distance: the tests' bounds).  ina_a also holds the float64 curve of the
PLAIN InstanceNorm network of its configuration (the yardstick of the bf16 test).  No reference source is copied.
"""
import functools
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, MODEL_SEED, LR, NSAMP, make_inputs, probe      # noqa: E402
from make_golden_bn import KEYS, store_state, trainer_for, double_losses    # noqa: E402

AFFINE_SEED = 4321

CONFIGS = {
    'ina_a': dict(in_nc=3, out_nc=1, nf=4, ndf=4, n_layers=3, norm=False, activation='leakyrelu', final_act='sigmoid',
                  loss_type='tversky', B=2, size=256, steps=10, plain64=True),
    'ina_b': dict(in_nc=3, out_nc=3, nf=4, ndf=4, n_layers=3, norm=True, activation='tanh', final_act='softmax',
                  loss_type='weighted_bce', B=2, size=256, steps=10),
}


def build(cfg, affine=True):
    from patchgan import UNet, Discriminator
    norm_layer = functools.partial(nn.InstanceNorm2d, affine=True) if affine else nn.InstanceNorm2d
    torch.manual_seed(MODEL_SEED)
    g = UNet(cfg['in_nc'], cfg['out_nc'], cfg['nf'], norm_layer=norm_layer, use_dropout=False,
             activation=cfg['activation'], final_act=cfg['final_act'])
    d = Discriminator(cfg['in_nc'] + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=cfg['norm'], norm_layer=norm_layer)
    gen = torch.Generator().manual_seed(AFFINE_SEED)
    with torch.no_grad():
        for net in (g, d):
            for m in net.modules():
                if isinstance(m, nn.InstanceNorm2d) and m.affine:
                    m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                    m.bias.copy_(torch.rand(m.bias.shape, generator=gen) - 0.5)
    return g, d


def run64(cfg, nsteps, affine, out, prefix):
    """K steps in float64; with `out`, also the step-1 gradient probes, the state after step K and the evaluation losses."""
    g64, d64 = build(cfg, affine)
    g64, d64 = g64.double().train(), d64.double().train()
    gopt = torch.optim.Adam(g64.parameters(), lr=LR, betas=(0.9, 0.999))
    dopt = torch.optim.Adam(d64.parameters(), lr=LR, betas=(0.9, 0.999))
    x, y = make_inputs(cfg)
    x64, y64 = x.double(), y.double()
    curve = []
    for s in range(nsteps):
        curve.append(double_losses(g64, d64, x64, y64, cfg, gopt, dopt))
        if s == 0 and out is not None:
            for k, p in g64.named_parameters():
                out['ggrad1_64/' + k] = probe(p.grad)
            for k, p in d64.named_parameters():
                out['dgrad1_64/' + k] = probe(p.grad)
    if out is not None:
        for k, v in g64.state_dict().items():
            out['gK64/' + k] = probe(v)
        for k, v in d64.state_dict().items():
            out['dK64/' + k] = probe(v)
        with torch.no_grad():
            out['eval_losses64'] = np.array(double_losses(g64, d64, x64, y64, cfg, gopt, dopt, train=False))
    return np.array(curve, dtype=np.float64)


def run_config(name, cfg):
    cfg = dict(cfg)
    nsteps = cfg.pop('steps')
    plain64 = cfg.pop('plain64', False)
    sys.path.insert(0, REF)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g, d = build(cfg)
    out = {}
    store_state(out, 'g0/', g.state_dict(), True)
    store_state(out, 'd0/', d.state_dict(), True)
    x, y = make_inputs(cfg)
    g.train()
    d.train()
    with torch.no_grad():
        gen0, hid0 = g(x, return_hidden=True)
        out['fwd/gen'] = probe(gen0)
        out['fwd/hidden'] = probe(hid0)
        out['fwd/disc_fake'] = probe(d(torch.cat((x, gen0), 1)))
        g64, d64 = build(cfg)
        g64, d64 = g64.double().train(), d64.double().train()
        gen64, hid64 = g64(x.double(), return_hidden=True)
        out['fwd64/gen'] = probe(gen64)
        out['fwd64/hidden'] = probe(hid64)
        out['fwd64/disc_fake'] = probe(d64(torch.cat((x.double(), gen64), 1)))

    t = trainer_for(g, d, cfg)
    curve = []
    for s in range(nsteps):
        l = t.batch(x, y, train=True)
        curve.append([l[k] for k in KEYS])
        if s == 0:
            for k, p in g.named_parameters():
                out['ggrad1/' + k] = probe(p.grad)
            for k, p in d.named_parameters():
                out['dgrad1/' + k] = probe(p.grad)
    out['losses'] = np.array(curve, dtype=np.float64)
    for k, v in g.state_dict().items():
        out['gK/' + k] = probe(v)
    for k, v in d.state_dict().items():
        out['dK/' + k] = probe(v)
    l = t.batch(x, y, train=False)
    out['eval_losses'] = np.array([l[k] for k in KEYS])

    out['losses64'] = run64(cfg, nsteps, True, out, '')
    if plain64:
        out['plain_losses64'] = run64(cfg, nsteps, False, None, '')

    out['cfg_keys'] = np.array(list(cfg.keys()))
    out['cfg_vals'] = np.array([str(v) for v in cfg.values()])
    out['meta'] = np.array([MODEL_SEED, nsteps, NSAMP, AFFINE_SEED])
    path = os.path.join(HERE, f'{name}.npz')
    np.savez_compressed(path, **out)
    err = np.abs(out['losses'] - out['losses64']).max()
    print(name, 'loss[0]', curve[0][0], 'loss[-1]', curve[-1][0], 'max |fp32 - fp64|', err, os.path.getsize(path), 'bytes',
          flush=True)


if __name__ == '__main__':
    names = sys.argv[1:] or list(CONFIGS)
    for n in names:
        run_config(n, CONFIGS[n])
