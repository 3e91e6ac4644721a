"""Cost of Trainer.diffaug at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on one MI355X: ONE process, two trainers over
the same networks' configuration -- the option off and on ('flip,translation,cutout') -- alternated ROUNDS times, STEPS timed steps per
leg and round (each trainer's launch mode is decided and settled before the first timed round).  Then the three kernels on their own
from HIP events at the step's shapes: pg_diffaug_params for N = 16, pg_diffaug_fwd on one half of din (N = 16, 4 channels) and
pg_diffaug_bwd on the generator's channel of D's input gradient (a 1-channel slice of a 4-float pixel into a dense view), with the bytes
each moves and the rate that gives.  Prints one JSON line.  (Off against the parent commit: tools/ab.sh with bench.py.)"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('STEPS', '20'))
POLICY = os.environ.get('POLICY', 'flip,translation,cutout')
cfg = CONFIGS['cfg2']
dev = torch.device('cuda', 0)
x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))


def trainer(policy):
    torch.manual_seed(1234)
    G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
    D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False).to(dev)
    t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgaug_'))
    t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = cfg['loss_type'], 200, True, 'auto'
    t.diffaug = policy
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


legs = {'off': trainer(None), 'on': trainer(POLICY)}
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


N, H, W = cfg['batch'], x.shape[2], x.shape[3]
Cd, Cout = 3 + cfg['out_nc'], cfg['out_nc']
counter = torch.zeros(1, dtype=torch.int64, device=dev)
table = E.diffaug_params(0, counter, 0, E.diffaug_policy(POLICY), 0, N, H, W)
din, aug = E.View.alloc(2 * N, H, W, Cd, dev, zero=True), E.View.alloc(2 * N, H, W, Cd, dev)
ddin, dgen = E.View.alloc(N, H, W, Cd, dev, zero=True), E.View.alloc(N, H, W, Cout, dev)
fwd_bytes, bwd_bytes = 2 * N * H * W * Cd * 4, 2 * N * H * W * Cout * 4
kern = {'params_ms': events(lambda: E.diffaug_params(0, counter, 0, 7, 0, N, H, W, params=table)),
        'fwd_half_ms': events(lambda: E.diffaug_fwd(din.samples(0, N), aug.samples(0, N), table)),
        'bwd_ms': events(lambda: E.diffaug_bwd(ddin.channels(Cd - Cout, Cout), dgen, table)),
        'fwd_half_bytes': fwd_bytes, 'bwd_bytes': bwd_bytes}
kern['fwd_half_TBps'] = round(fwd_bytes / kern['fwd_half_ms'] / 1e9, 2)
kern['bwd_TBps'] = round(bwd_bytes / kern['bwd_ms'] / 1e9, 2)
print(json.dumps({'metric': f'cfg2 training step with Trainer.diffaug = {POLICY!r}, ms per step (median of rounds; min..max)',
                  'rounds': ROUNDS, 'steps_per_round': STEPS, 'launch_mode': modes,
                  'ms_per_step': {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  'kernels': kern}))
