"""Cost of Trainer.betas + Trainer.weight_decay at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on one MI355X: ONE process,
three trainers over the same network configuration -- two default ones (their difference is the run-to-run spread of this tool) and one
with betas = ((0.5, 0.999), (0.0, 0.9)), weight_decay = (1e-2, 1e-2) -- alternated ROUNDS times, STEPS timed steps per leg and round
(each trainer's launch mode is decided and settled before the first timed round).  Then the Adam(G) launch on its own from HIP events
on the generator's flat buffers: pg_adam_step against pg_adamw_step (28 bytes per parameter either way; the decay is one multiply).
Prints one JSON line.  (The default step against the parent commit's: tools/ab.sh <parent tree> <this tree> <rounds>.)"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('STEPS', '20'))
cfg = CONFIGS['cfg2']
dev = torch.device('cuda', 0)
x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))


def trainer(optim):
    torch.manual_seed(1234)
    G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
    D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False).to(dev)
    t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgopt_'))
    t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = cfg['loss_type'], 200, True, 'auto'
    if optim:
        t.betas, t.weight_decay = ((0.5, 0.999), (0.0, 0.9)), (1e-2, 1e-2)
    t.setup_optimizers(1e-3, 1e-3)
    G.train()
    D.train()
    return t


def run(t, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        t.batch(x, y, train=True)
    t.flush()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


legs = {'default': trainer(False), 'default_again': trainer(False), 'betas_decay': trainer(True)}
settle = 3 * (2 * pg.Trainer.TRIAL_STEPS + 2) + 4 + 48
modes = {}
for name, t in legs.items():
    run(t, settle)
    modes[name] = t.launch_mode
ms = {k: [] for k in legs}
for r in range(ROUNDS):
    for name, t in legs.items():
        run(t, 2)
        ms[name].append(run(t, STEPS))


def events(fn, reps=50):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    v = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


n = legs['default'].generator.flat.numel()
p, g, m, v = (torch.randn(n, device=dev) * s for s in (0.02, 1e-3, 1e-3, 0.0))
v = v + 1e-6
kern = {'parameters': n,
        'adam_ms': events(lambda: E.adam_update(p, g, m, v, step=100, lr=1e-3)),
        'adam_again_ms': events(lambda: E.adam_update(p, g, m, v, step=100, lr=1e-3)),
        'adamw_ms': events(lambda: E.adam_update(p, g, m, v, step=100, lr=1e-3, weight_decay=1e-2, beta1=0.5, beta2=0.999))}
kern['adamw_tb_per_s'] = round(28.0 * n / (kern['adamw_ms'][0] * 1e-3) / 1e12, 3)
med = {k: statistics.median(val) for k, val in ms.items()}
print(json.dumps({'metric': 'cfg2 training step, betas + weight_decay set for both networks against the default step, ms per step '
                            '(median of rounds; min..max)',
                  'rounds': ROUNDS, 'steps_per_round': STEPS, 'launch_mode': modes,
                  'ms_per_step': {k: [round(statistics.median(val), 3), round(min(val), 3), round(max(val), 3)] for k, val in ms.items()},
                  'default_vs_default_again_ms': round(abs(med['default'] - med['default_again']), 3),
                  'betas_decay_minus_default_ms': round(med['betas_decay'] - min(med['default'], med['default_again']), 3),
                  'adam_g_launch_ms_median_min_max': kern}))
