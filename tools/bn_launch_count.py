"""Kernel dispatches per training step, InstanceNorm vs BatchNorm networks at cfg2's shape, counted by the profiler:

  rocprofv3 --kernel-trace --stats -d OUT -o k --output-format csv -- python tools/bn_launch_count.py run [--steps 5]
  python tools/bn_launch_count.py parse OUT

`run` warms up four trainers (InstanceNorm / BatchNorm generator, each with a discriminator without and with norm) and then steps each
of them `--steps` times launch by launch on one stream, a marker dispatch (a cumulative sum, a kernel the step never launches) before
and after every block.  `parse` reads the kernel trace, orders the dispatches by their dispatch id and prints one JSON line: dispatches
per step of each run between its markers, and the BatchNorm-minus-InstanceNorm differences."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile

RUNS = [('in', False), ('bn', False), ('in', True), ('bn', True)]
MARK = 'scan'          # (torch.cumsum's kernels carry it in their names)


def run(steps):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from torch import nn
    import patchgan_amd as pg
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(16, 3, 256, 256, generator=gen).cuda()
    y = (torch.rand(16, 1, 256, 256, generator=gen) > 0.7).float().cuda()
    ts = []
    for kind, dnorm in RUNS:
        nl = nn.BatchNorm2d if kind == 'bn' else nn.InstanceNorm2d
        torch.manual_seed(1234)
        g = pg.UNet(3, 1, 64, norm_layer=nl, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
        d = pg.Discriminator(4, 64, n_layers=3, norm=dnorm, norm_layer=nl).cuda()
        t = pg.Trainer(g, d, tempfile.mkdtemp())
        t.loss_type, t.seg_alpha = 'tversky', 200
        t.setup_optimizers(1e-3, 1e-3)
        for _ in range(4):          # kernel plans, weight-cache plans (from the second step on: one batched preparation), workspaces
            t.batch(x, y, train=True)
        ts.append(t)
    torch.cuda.synchronize()
    one = torch.ones(7, device='cuda')
    for t in ts:
        torch.cumsum(one, 0)
        for _ in range(steps):
            t.batch(x, y, train=True)
        t.flush()
        torch.cuda.synchronize()
    torch.cumsum(one, 0)
    torch.cuda.synchronize()
    print(json.dumps({'steps': steps}))


def parse(root, steps):
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, f'no kernel trace under {root}'
    rows = []
    for f in files:
        with open(f) as fh:
            rows += [(int(r['Dispatch_Id']), r['Kernel_Name']) for r in csv.DictReader(fh)]
    rows.sort()
    # the dispatches between consecutive markers (a marker may be more than one dispatch: a run of marker kernels counts once)
    blocks, cur, in_mark = [], None, False
    for _, name in rows:
        if MARK in name:
            if not in_mark and cur is not None:
                blocks.append(cur)
            cur, in_mark = 0, True
        else:
            in_mark = False
            if cur is not None:
                cur += 1
    assert len(blocks) >= len(RUNS), (len(blocks), 'blocks between markers')
    per = {}
    for (kind, dnorm), n in zip(RUNS, blocks[-len(RUNS):]):
        per[f"{kind}{'_dnorm' if dnorm else ''}"] = n / steps
    out = {'shape': 'cfg2 (256x256x3 -> 1, bs 16, nf = ndf = 64), one stream', 'steps': steps, 'dispatches_per_step': per,
           'bn_minus_in': per['bn'] - per['in'], 'bn_minus_in_dnorm': per['bn_dnorm'] - per['in_dnorm']}
    print(json.dumps(out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['run', 'parse'])
    ap.add_argument('root', nargs='?')
    ap.add_argument('--steps', type=int, default=5)
    a = ap.parse_args()
    run(a.steps) if a.what == 'run' else parse(a.root, a.steps)
