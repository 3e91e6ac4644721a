"""Cost of Trainer.clip_grad_norm at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on one MI355X: ONE process, one
trainer, the legs off / inf (monitor) / a clipping value alternated ROUNDS times, STEPS timed steps per leg and round (each leg is a
kind of step of its own: its launch mode is decided and settled before the first timed round).  Then the kernels on their own from
HIP events: pg_grad_norm and pg_adam_step / pg_adam_clip_step on the generator's and the discriminator's flat buffers.
Prints one JSON line."""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('STEPS', '20'))
cfg = CONFIGS['cfg2']
dev = torch.device('cuda', 0)
torch.manual_seed(1234)
G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False).to(dev)
t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgclip_'))
t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = cfg['loss_type'], 200, True, 'auto'
t.setup_optimizers(1e-3, 1e-3)
G.train()
D.train()
x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))


def run(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        t.batch(x, y, train=True)
    t.flush()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


# the monitor leg first: its norms give the clipping value (a quarter of the smaller of the last norms)
settle = 3 * (2 * t.TRIAL_STEPS + 2) + 4 + 48
t.clip_grad_norm = float('inf')
run(settle)
s = t.read_grad_stats()
clip = (0.25 * s['gen']['norm'], 0.25 * s['disc']['norm'])
legs = {'off': None, 'inf': float('inf'), 'clip': clip}
modes = {}
for name, v in legs.items():
    t.clip_grad_norm = v
    run(settle)
    modes[name] = t.launch_mode
ms = {k: [] for k in legs}
for r in range(ROUNDS):
    for name, v in legs.items():
        t.clip_grad_norm = v
        run(2)
        ms[name].append(run(STEPS))
t.clip_grad_norm = clip
stats = t.read_grad_stats()


def events(fn, reps=20):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return round(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps)), 4)


kern = {}
for name, net in (('G', G), ('D', D)):
    n = net.flat.numel()
    g = net.grad_flat
    p, m, v = (torch.zeros_like(net.flat) for _ in range(3))
    ws = torch.zeros(E.grad_norm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    stat = torch.zeros(8, dtype=torch.float64, device=dev)
    kern[name] = {'parameters': n,
                  'grad_norm_ms': events(lambda: E.grad_norm(g, 1e30, ws, stat)),
                  'adam_step_ms': events(lambda: E.adam_update(p, g, m, v, step=10, lr=1e-3)),
                  'adam_clip_step_ms': events(lambda: E.adam_update(p, g, m, v, step=10, lr=1e-3, stat=stat))}
    kern[name]['grad_norm_GBps'] = round(4 * n / kern[name]['grad_norm_ms'] / 1e6, 1)
print(json.dumps({'metric': 'cfg2 training step with Trainer.clip_grad_norm, ms per step (median of rounds; min..max)',
                  'rounds': ROUNDS, 'steps_per_round': STEPS, 'launch_mode': modes, 'clip_values': [round(c, 5) for c in clip],
                  'ms_per_step': {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  'last_stats': {k: {a: stats[k][a] for a in ('norm', 'coef', 'clipped', 'steps', 'skipped')} for k in stats},
                  'kernels': kern}))
