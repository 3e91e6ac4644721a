"""Cost of Discriminator(spectral_norm=True) at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on one MI355X: ONE process,
two trainers over the same generator configuration -- the discriminator without and with the option -- alternated ROUNDS times,
STEPS timed steps per leg and round (each trainer's launch mode is decided and settled before the first timed round).  Then the two
launch sequences on their own from HIP events: pg_spectral_fwd (iterating and not) and pg_spectral_bwd on the discriminator's five
layers.  Prints one JSON line."""
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


def trainer(spectral):
    torch.manual_seed(1234)
    G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
    D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False, spectral_norm=spectral).to(dev)
    t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgsn_'))
    t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = cfg['loss_type'], 200, True, 'auto'
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


legs = {'off': trainer(False), 'on': trainer(True)}
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


D = legs['on'].discriminator
g = torch.randn_like(D.flat) * 1e-3
kern = {'parameters': D.flat.numel(), 'layers': [(l.a, l.b) for l in D.engine.layers],
        'fwd_iterate_ms': events(lambda: D.spectral_normalize(True)),
        'fwd_fixed_ms': events(lambda: D.spectral_normalize(False)),
        'bwd_ms': events(lambda: D.spectral_grad_map(g))}
print(json.dumps({'metric': 'cfg2 training step with Discriminator(spectral_norm=True), ms per step (median of rounds; min..max)',
                  'rounds': ROUNDS, 'steps_per_round': STEPS, 'launch_mode': modes,
                  'ms_per_step': {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  'kernels': kern}))
