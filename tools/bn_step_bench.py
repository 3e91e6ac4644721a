"""InstanceNorm vs BatchNorm generator in the training step at cfg2's shape (256 x 256 x 3 -> 1 mask, bs 16, nf = ndf = 64,
leakyrelu / sigmoid / tversky): python tools/bn_step_bench.py [--steps 20] [--blocks 3] [--mode eager1|eager2|graph]
(needs the gfx950 build).  In one process, on identical inputs, the two generators' Trainer.batch(train=True) steps alternate in
blocks after a warm-up of every shape; the same pair again with a discriminator with norm=True (its norm the generator's).  Every
run is launched the same way (Trainer.AUTO_FORCE = --mode).  Prints one JSON line: ms per step of each run, the BN / IN ratios and
the C ABI calls per step (each launches one to three kernels), counted launch by launch."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402
from torch import nn                           # noqa: E402
import patchgan_amd as pg                      # noqa: E402
from patchgan_amd import _lib as L             # noqa: E402


def make(norm_layer, dnorm, mode):
    torch.manual_seed(1234)
    g = pg.UNet(3, 1, 64, norm_layer=norm_layer, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
    d = pg.Discriminator(4, 64, n_layers=3, norm=dnorm, norm_layer=norm_layer).cuda()
    t = pg.Trainer(g, d, tempfile.mkdtemp())
    t.loss_type, t.seg_alpha = 'tversky', 200
    t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    t.setup_optimizers(1e-3, 1e-3)
    g.train()
    d.train()
    return t


class _Counter:
    """Counts the C ABI calls that launch kernels during one step (every pg_* entry point taking a stream, except queries)."""
    def __init__(self):
        self.n = 0

    def __enter__(self):
        lib = L.load()
        self.saved = {}
        for name in L.SIGNATURES:
            if name.endswith(('_bytes', '_count', '_chunks', '_ok', '_kernel', '_flops', '_describe', '_nc', '_doubles')) \
                    or name in ('pg_version', 'pg_conv_time_next', 'pg_conv_time_next2', 'pg_conv_max_tensor_bytes'):
                continue
            fn = getattr(lib, name)
            self.saved[name] = fn

            def wrap(*a, _fn=fn):
                self.n += 1
                return _fn(*a)
            setattr(lib, name, wrap)
        return self

    def __exit__(self, *exc):
        lib = L.load()
        for name, fn in self.saved.items():
            setattr(lib, name, fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--mode', default='eager2')
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(16, 3, 256, 256, generator=gen).cuda()
    y = (torch.rand(16, 1, 256, 256, generator=gen) > 0.7).float().cuda()
    runs = {(k, dn): make(nl, dn, a.mode) for dn in (False, True) for k, nl in (('in', nn.InstanceNorm2d), ('bn', nn.BatchNorm2d))}
    launches = {}
    for key, t in runs.items():               # warm-up: kernel plans, weight-cache plans, workspaces, the launch decision
        for _ in range(8):
            t.batch(x, y, train=True)
        t.flush()
        torch.cuda.synchronize()
        t.AUTO_FORCE = None
        t.two_streams, t.graph = (a.mode == 'eager2'), False      # count launch by launch
        with _Counter() as c:
            t.batch(x, y, train=True)
        t.flush()
        launches[key] = c.n
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', a.mode
    ms = {k: [] for k in runs}
    for _ in range(a.blocks):
        for key, t in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                t.batch(x, y, train=True)
            t.flush()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) / a.steps * 1e3)
    best = {k: min(v) for k, v in ms.items()}
    name = lambda k: f"{k[0]}{'_dnorm' if k[1] else ''}"
    out = {'shape': 'cfg2 (256x256x3 -> 1, bs 16, nf = ndf = 64)', 'launch_mode': [runs[k].launch_mode for k in runs][0],
           'steps_per_block': a.steps, 'blocks': a.blocks,
           'ms_per_step': {name(k): round(v, 4) for k, v in best.items()},
           'ms_per_block': {name(k): [round(x, 4) for x in v] for k, v in ms.items()},
           'ratio_bn_over_in': round(best[('bn', False)] / best[('in', False)], 4),
           'ratio_bn_over_in_dnorm': round(best[('bn', True)] / best[('in', True)], 4),
           'abi_calls_per_step': {name(k): v for k, v in launches.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
