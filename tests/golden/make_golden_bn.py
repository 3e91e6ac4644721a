#!/usr/bin/env python3
"""Generate the BatchNorm2d golden fixtures by IMPORTING THE REFERENCE (build container only), like make_golden.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bn.py [name ...]

Only DATA is written to ``tests/golden/bn_*.npz``: the initial state_dicts (key order, shapes, dtypes; values in full for small
tensors, probes otherwise), forward probes at the initial weights in training mode, K steps of the reference's Trainer.batch with
gradient / running-statistics probes after step 1, the state after step K, the two kinds of batch(train=False) after it, and the
same K steps in float64 (the reference's own fp32-vs-float64 distance: the tests' bounds).  No reference source is copied.
"""
import contextlib
import copy
import io
import os
import sys
import tempfile

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, MODEL_SEED, LR, NSAMP, make_inputs, probe      # noqa: E402

KEYS = ['gen', 'gen_loss', 'gdisc', 'discr', 'discf', 'disc']
FULL_MAX = 4096          # tensors up to this many elements are stored in full, larger ones as probes

CONFIGS = {
    'bn_a': dict(in_nc=3, out_nc=1, nf=4, ndf=4, n_layers=3, norm=False, activation='leakyrelu', final_act='sigmoid',
                 loss_type='tversky', B=4, size=256, steps=10),
    'bn_b': dict(in_nc=3, out_nc=3, nf=4, ndf=4, n_layers=3, norm=True, activation='tanh', final_act='softmax',
                 loss_type='weighted_bce', B=2, size=256, steps=10),
    'bn_c': dict(in_nc=3, out_nc=1, nf=8, ndf=4, n_layers=5, norm=True, activation='relu', final_act='sigmoid',
                 loss_type='MAE', B=2, size=128, steps=10),
    'bn_w_cfg2': dict(in_nc=3, out_nc=1, nf=64, ndf=64, n_layers=3, norm=False, activation='leakyrelu', final_act='sigmoid',
                      loss_type='tversky', B=16, size=256, steps=4, probes_only=True),
}


def build(cfg):
    from patchgan import UNet, Discriminator
    torch.manual_seed(MODEL_SEED)
    g = UNet(cfg['in_nc'], cfg['out_nc'], cfg['nf'], norm_layer=nn.BatchNorm2d, use_dropout=False,
             activation=cfg['activation'], final_act=cfg['final_act'])
    d = Discriminator(cfg['in_nc'] + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=cfg['norm'],
                      norm_layer=nn.BatchNorm2d)
    return g, d


def store_state(out, prefix, sd, full):
    out[prefix + 'keys'] = np.array(list(sd.keys()))
    out[prefix + 'shapes'] = np.array([','.join(str(s) for s in v.shape) for v in sd.values()])
    out[prefix + 'dtypes'] = np.array([str(v.dtype) for v in sd.values()])
    for k, v in sd.items():
        if full and v.numel() <= FULL_MAX:
            out[prefix + 'full/' + k] = v.detach().numpy().copy()
        else:
            out[prefix + 'probe/' + k] = probe(v)


def running_probes(out, prefix, net):
    for k, v in net.state_dict().items():
        if 'running_' in k or 'num_batches_tracked' in k:
            out[prefix + k] = probe(v) if v.dim() else np.array([v.item()], dtype=np.float64)


def trainer_for(g, d, cfg):
    from patchgan import Trainer
    with contextlib.redirect_stdout(io.StringIO()):
        t = Trainer(g, d, tempfile.mkdtemp(), device='cpu')
    t.loss_type = cfg['loss_type']
    t.seg_alpha = 200
    t.gen_optimizer = torch.optim.Adam(g.parameters(), lr=LR, betas=(0.9, 0.999))
    t.disc_optimizer = torch.optim.Adam(d.parameters(), lr=LR, betas=(0.9, 0.999))
    return t


def double_losses(g, d, x, y, cfg, gopt, dopt, train=True):
    """One step of trainer.py:50-115 in float64 (the reference's Trainer.batch builds float32 labels, which BCELoss refuses next to
    double inputs): the same operations in the same order on the .double() modules; train=False skips the updates as batch() does."""
    from patchgan.losses import fc_tversky, MAE_loss
    from torch.nn.functional import binary_cross_entropy
    bce = nn.BCELoss()
    gen_img = g(x)
    disc_fake = d(torch.cat((x, gen_img), 1))
    ones = torch.ones_like(disc_fake)
    zeros = torch.zeros_like(disc_fake)
    if cfg['loss_type'] == 'tversky':
        gen_loss = fc_tversky(y, gen_img, beta=0.75, gamma=0.75) * 200
    elif cfg['loss_type'] == 'weighted_bce':
        if gen_img.shape[1] > 1:
            weight = 1 - torch.sum(y, dim=(2, 3), keepdim=True) / torch.sum(y)
        else:
            weight = torch.ones_like(y)
        gen_loss = binary_cross_entropy(gen_img, y, weight=weight) * 200
    else:
        gen_loss = MAE_loss(gen_img, y) * 200
    gen_loss_disc = bce(disc_fake, ones)
    gen_loss = gen_loss + gen_loss_disc
    if train:
        g.zero_grad()
        gen_loss.backward()
        gopt.step()
        d.zero_grad()
    disc_real = d(torch.cat((x, y), 1))
    disc_fake = d(torch.cat((x, gen_img.detach()), 1))
    loss_real = bce(disc_real, ones)
    loss_fake = bce(disc_fake, zeros)
    disc_loss = (loss_fake + loss_real) / 2.
    if train:
        disc_loss.backward()
        dopt.step()
    return [gen_loss.item(), gen_loss.item(), gen_loss_disc.item(), loss_real.item(), loss_fake.item(), disc_loss.item()]


def run_config(name, cfg):
    cfg = dict(cfg)
    nsteps = cfg.pop('steps')
    full = not cfg.pop('probes_only', False)
    sys.path.insert(0, REF)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g, d = build(cfg)
    out = {}
    store_state(out, 'g0/', g.state_dict(), full)
    store_state(out, 'd0/', d.state_dict(), full)
    x, y = make_inputs(cfg)

    # forward probes at the initial weights in training mode -- on copies: a training-mode forward moves the running statistics
    gc, dc = copy.deepcopy(g), copy.deepcopy(d)
    gc.train()
    dc.train()
    with torch.no_grad():
        gen0, hid0 = gc(x, return_hidden=True)
        out['fwd/gen'] = probe(gen0)
        out['fwd/hidden'] = probe(hid0)
        out['fwd/disc_fake'] = probe(dc(torch.cat((x, gen0), 1)))
    running_probes(out, 'fwd_run/g/', gc)
    running_probes(out, 'fwd_run/d/', dc)

    t = trainer_for(g, d, cfg)
    g.train()
    d.train()
    curve = []
    for s in range(nsteps):
        l = t.batch(x, y, train=True)
        curve.append([l[k] for k in KEYS])
        if s == 0:
            for k, p in g.named_parameters():
                out['ggrad1/' + k] = probe(p.grad)
            for k, p in d.named_parameters():
                out['dgrad1/' + k] = probe(p.grad)
            running_probes(out, 'run1/g/', g)
            running_probes(out, 'run1/d/', d)
    out['losses'] = np.array(curve, dtype=np.float64)
    for k, v in g.state_dict().items():
        out['gK/' + k] = probe(v)
    for k, v in d.state_dict().items():
        out['dK/' + k] = probe(v)
    # batch(train=False) with the modules left in training mode: batch statistics, the running statistics move, no parameter update
    l = t.batch(x, y, train=False)
    out['trainmode_eval_losses'] = np.array([l[k] for k in KEYS])
    running_probes(out, 'trainmode_eval_run/g/', g)
    running_probes(out, 'trainmode_eval_run/d/', d)
    # ... and in evaluation mode: the running statistics
    g.eval()
    d.eval()
    l = t.batch(x, y, train=False)
    out['eval_losses'] = np.array([l[k] for k in KEYS])
    with torch.no_grad():
        out['eval_gen'] = probe(g(x))

    # the same K steps in float64 (bounds for the tests: the reference's own fp32-vs-float64 distance)
    g64, d64 = build(cfg)
    g64, d64 = g64.double(), d64.double()
    g64.train()
    d64.train()
    gopt = torch.optim.Adam(g64.parameters(), lr=LR, betas=(0.9, 0.999))
    dopt = torch.optim.Adam(d64.parameters(), lr=LR, betas=(0.9, 0.999))
    x64, y64 = x.double(), y.double()
    curve64 = []
    for s in range(nsteps):
        curve64.append(double_losses(g64, d64, x64, y64, cfg, gopt, dopt))
        if s == 0:
            for k, p in g64.named_parameters():
                out['ggrad1_64/' + k] = probe(p.grad)
            for k, p in d64.named_parameters():
                out['dgrad1_64/' + k] = probe(p.grad)
            running_probes(out, 'run1_64/g/', g64)
            running_probes(out, 'run1_64/d/', d64)
    out['losses64'] = np.array(curve64, dtype=np.float64)
    # the same post-K sequence in float64: the bounds of the tests' checks after step K
    with torch.no_grad():
        out['trainmode_eval_losses64'] = np.array(double_losses(g64, d64, x64, y64, cfg, gopt, dopt, train=False))
    running_probes(out, 'trainmode_eval_run64/g/', g64)
    running_probes(out, 'trainmode_eval_run64/d/', d64)
    g64.eval()
    d64.eval()
    with torch.no_grad():
        out['eval_losses64'] = np.array(double_losses(g64, d64, x64, y64, cfg, gopt, dopt, train=False))
        out['eval_gen64'] = probe(g64(x64))

    out['cfg_keys'] = np.array(list(cfg.keys()))
    out['cfg_vals'] = np.array([str(v) for v in cfg.values()])
    out['meta'] = np.array([MODEL_SEED, nsteps, NSAMP])
    path = os.path.join(HERE, f'{name}.npz')
    np.savez_compressed(path, **out)
    err = np.abs(out['losses'] - out['losses64']).max()
    print(name, 'loss[0]', curve[0][0], 'loss[-1]', curve[-1][0], 'max |fp32 - fp64|', err, os.path.getsize(path), 'bytes',
          flush=True)


if __name__ == '__main__':
    names = sys.argv[1:] or list(CONFIGS)
    for n in names:
        run_config(n, CONFIGS[n])
