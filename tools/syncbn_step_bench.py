"""What synchronised BatchNorm costs in the training step at the bn_w_cfg2 shape (cfg2 with BatchNorm: 256 x 256 x 3 -> 1 mask,
bs 16, nf = ndf = 64, leakyrelu / sigmoid / tversky, a discriminator without norm):
    python tools/syncbn_step_bench.py --kind syncbn --group nccl1      a SyncBatchNorm pair under a ONE-rank RCCL group with
                                                                       PATCHGAN_DP_FORCE=1 (no peer: a lower bound of the collectives' cost)
    python tools/syncbn_step_bench.py --kind bn                        a BatchNorm2d pair, no group
(needs the gfx950 build; each call is one process and one leg -- alternate the calls and take medians, a process group cannot be
left and re-entered inside one process without moving the other leg).  Drives Trainer.batch(train=True) directly with the
trainer's default launch settings, on device-resident inputs: `--warmup` steps, then `--steps` timed ones between two device
synchronisations.  Prints one JSON line: ms per step, the launch mode, and the collectives of one step (all of them, and those of
the BatchNorm layers: one per layer and pass, forward and backward)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', choices=('bn', 'syncbn'), default='bn')
    ap.add_argument('--group', choices=('none', 'nccl1'), default='none')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    a = ap.parse_args()
    if a.group == 'nccl1':
        os.environ['PATCHGAN_DP_FORCE'] = '1'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
    import patchgan_amd as pg                  # (before HIP is initialised: the package sets its hardware-queue default)
    import torch
    from torch import nn
    from patchgan_amd import engine as E, parallel
    if a.group == 'nccl1':
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        norm_layer = nn.SyncBatchNorm if a.kind == 'syncbn' else nn.BatchNorm2d
        torch.manual_seed(1234)
        g = pg.UNet(3, 1, 64, norm_layer=norm_layer, use_dropout=False, activation='leakyrelu', final_act='sigmoid').cuda()
        d = pg.Discriminator(4, 64, n_layers=3, norm=False, norm_layer=norm_layer).cuda()
        t = pg.Trainer(g, d, tempfile.mkdtemp())
        t.loss_type, t.seg_alpha = 'tversky', 200
        t.setup_optimizers(1e-3, 1e-3)
        g.train()
        d.train()
        gen = torch.Generator().manual_seed(7)
        x = torch.rand(16, 3, 256, 256, generator=gen).cuda()
        y = (torch.rand(16, 1, 256, 256, generator=gen) > 0.7).float().cuda()
        for _ in range(a.warmup):
            t.batch(x, y, train=True)
        t.flush()
        torch.cuda.synchronize()
        # the collectives of one step, counted call by call
        ds = parallel.current()
        counts = {'all': 0, 'bn': 0}
        side, bn_side = ds.all_reduce_side, getattr(E, '_bn_allreduce', None)      # (None: a tree without the split route)

        def counted(*args, **kw):
            counts['all'] += 1
            return side(*args, **kw)

        def bn_counted(*args, **kw):
            counts['bn'] += 1
            return bn_side(*args, **kw)
        ds.all_reduce_side, E._bn_allreduce = counted, bn_counted
        try:
            t.batch(x, y, train=True)
            t.flush()
        finally:
            ds.all_reduce_side, E._bn_allreduce = side, bn_side
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            t.batch(x, y, train=True)
        t.flush()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        print(json.dumps({'shape': 'bn_w_cfg2 (256x256x3 -> 1, bs 16, nf = ndf = 64)', 'kind': a.kind, 'group': a.group,
                          'data_parallel_path': bool(ds.on), 'launch_mode': t.launch_mode, 'steps': a.steps,
                          'ms_per_step': round(ms, 4), 'collectives_per_step': counts['all'] if ds.on else 0,
                          'batchnorm_collectives_per_step': counts['bn']}))
    finally:
        if a.group == 'nccl1':
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == '__main__':
    main()
