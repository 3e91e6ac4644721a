"""Cost of Trainer.accumulate at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on one MI355X: ONE process, three trainers
over the same network configuration -- two default ones (their difference is the run-to-run spread of this tool) and one with
accumulate = 2 -- alternated ROUNDS times, STEPS timed calls per leg and round (each trainer's launch modes are decided and settled
before the first timed round).  The accumulating leg's calls are also timed one by one from HIP events at the start of each call, so
its 'begin' calls (no Adam launch: one 8-byte pass per network instead) and its 'close' calls (a 12-byte pass in front of Adam) are
reported separately.  Then pg_grad_accum on its own, mode by mode, on buffers of the generator's size, beside pg_adam_step at the same
size in the same run: achieved bytes per second, the Adam number being the yardstick.
Prints one JSON line.  (The default step against the parent commit's: tools/ab.sh <parent tree> <this tree> <rounds>.)"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('STEPS', '20'))
K = 2
cfg = CONFIGS['cfg2']
dev = torch.device('cuda', 0)
x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))


def trainer(accumulate):
    torch.manual_seed(1234)
    G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
    D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False).to(dev)
    t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgacc_'))
    t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = cfg['loss_type'], 200, True, 'auto'
    t.accumulate = accumulate
    t.setup_optimizers(1e-3, 1e-3)
    G.train()
    D.train()
    return t


def run(t, n, per_call=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    starts = []
    for _ in range(n):
        if per_call is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            starts.append((ev, E.accum_phase(t._acc_done, K)))
        t.batch(x, y, train=True)
    if per_call is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        starts.append((ev, None))
    t.flush()
    torch.cuda.synchronize()
    for (a, phase), (b, _) in zip(starts, starts[1:]):
        per_call[phase].append(a.elapsed_time(b))
    return (time.perf_counter() - t0) / n * 1e3


legs = {'default': trainer(None), 'default_again': trainer(None), 'accumulate_2': trainer(K)}
settle = 3 * (2 * pg.Trainer.TRIAL_STEPS + 2) + 4 + 48
modes = {}
for name, t in legs.items():
    run(t, settle * (K if t.accumulate else 1))          # (every phase is a kind of step of its own and is decided on its own)
    modes[name] = t.decided_modes() or [t.launch_mode]
ms = {k: [] for k in legs}
phase_ms = {'begin': [], 'close': []}
for r in range(ROUNDS):
    for name, t in legs.items():
        run(t, 2)
        ms[name].append(run(t, STEPS, phase_ms if t.accumulate else None))


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


def spread(v):
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


n = legs['default'].generator.flat.numel()
p, g, m, v, acc = (torch.randn(n, device=dev) * s for s in (0.02, 1e-3, 1e-3, 0.0, 1e-3))
v = v + 1e-6
g0 = g.clone()


def accum(mode):
    g.copy_(g0)          # (outside the timed launches: the closing modes overwrite g)
    return events(lambda: E.grad_accum(acc, g, mode, E.accum_scale(K)))


kern = {'parameters': n, 'adam_ms': events(lambda: E.adam_update(p, g, m, v, step=100, lr=1e-3))}
bytes_per = {'begin': 8, 'add': 12, 'close': 12, 'close_only': 8}
for mode in bytes_per:
    kern[mode + '_ms'] = accum(mode)
kern['adam_again_ms'] = events(lambda: E.adam_update(p, g, m, v, step=100, lr=1e-3))
kern['tb_per_s'] = dict({mode: round(b * n / (kern[mode + '_ms'][0] * 1e-3) / 1e12, 3) for mode, b in bytes_per.items()},
                        adam=round(28.0 * n / (min(kern['adam_ms'][0], kern['adam_again_ms'][0]) * 1e-3) / 1e12, 3))
med = {k: statistics.median(val) for k, val in ms.items()}
print(json.dumps({'metric': 'cfg2 training call with accumulate = 2 against the default step, ms per call (median of rounds; min..max); '
                            'per phase from HIP events at the start of each call',
                  'rounds': ROUNDS, 'calls_per_round': STEPS, 'launch_modes': modes,
                  'ms_per_call': {k: spread(val) for k, val in ms.items()},
                  'ms_per_phase': {k: spread(val) for k, val in phase_ms.items()},
                  'default_vs_default_again_ms': round(abs(med['default'] - med['default_again']), 3),
                  'accumulate_minus_default_ms': round(med['accumulate_2'] - min(med['default'], med['default_again']), 3),
                  'grad_accum_launch_ms_median_min_max': kern}))
