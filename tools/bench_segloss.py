"""Cost of the segmentation objectives beyond the reference's three (Trainer.loss_type = 'ce' | 'focal' | 'dice' | sums; segloss.hip) on
one MI355X, in ONE process.
  1. The two launches on their own, from HIP events, on the views of a cfg4 step (8 x 512 x 512, 4 classes: prediction and target 3
     floats into 8-float pixels, the gradient dense) and of a cfg2 step (16 x 256 x 256, one channel, 3 floats into 4-float pixels):
     pg_seg_loss_reduce + pg_seg_loss_value_grad for ce, focal, dice, ce+dice (cfg2: focal, dice, focal+dice) against the existing pair
     pg_loss_reduce_parts + pg_loss_value_grad with weighted_bce on the same views, alternated ROUNDS times (median of REPS calls per leg and
     round).  Bytes: what the pair must move (p and y twice, g once) and what it touches (whole pixels of the wider buffers).
  2. The cfg4-shape training step (fp32, graph = 'auto'): three trainers -- two with weighted_bce (their difference is the run-to-run
     spread of this tool) and one with ce+dice -- alternated ROUNDS times, STEPS timed steps per leg and round.
Prints one JSON line.  (The default step against the parent commit's: tools/ab.sh <parent tree> <this tree> <rounds>.)"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import _lib as L
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS, REPS = int(os.environ.get('ROUNDS', '3')), int(os.environ.get('STEPS', '10')), int(os.environ.get('REPS', '30'))
STEP = os.environ.get('STEP', '1') != '0'
dev = torch.device('cuda', 0)


def events(fn, reps):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))


def views(cfg):
    """(p, y, g) as a step of this configuration lays them out: the mask channels of the fake and real halves of one input buffer."""
    N, S, C = cfg['batch'], cfg['size'], cfg['out_nc']
    ld = 3 + C
    ld = -(-ld // 4) * 4
    gen = torch.Generator(device=dev).manual_seed(5)
    din = torch.rand(2 * N * S * S * ld, device=dev, generator=gen) * 0.98 + 0.01
    real = E.View(din, 0, ld, N, S, S, ld).channels(3, C)
    fake = E.View(din, N * S * S * ld, ld, N, S, S, ld).channels(3, C)
    y = (torch.rand(N, C, S, S, device=dev, generator=gen) > 0.7).float()
    din[:N * S * S * ld].view(N, S, S, ld)[..., 3:3 + C] = y.permute(0, 2, 3, 1)
    return fake, real, E.View.alloc(N, S, S, C, dev)


def pair_times(cfg, names):
    p, y, g = views(cfg)
    N = p.N
    loss = torch.empty(1, device=dev)
    final_act = 'softmax' if p.C > 1 else 'sigmoid'

    def new(name):
        spec = E.check_seg_loss(name, final_act, p.C)
        return lambda: E.seg_loss_finish(E.seg_loss_begin(p, y, spec), 200.0, g, loss, 0, N)

    def old():
        E.loss_finish(E.loss_begin(p, y, 0.0), L.LOSS_WBCE, 200.0, g, loss, 0, N)
    legs = dict({'weighted_bce (existing pair)': old}, **{n: new(n) for n in names})
    us = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            us[k].append(events(fn, REPS) * 1e3)
    npix = p.npix
    need = npix * p.C * 4 * 5                      # p and y in both launches, g once
    touched = npix * 4 * (4 * p.ld + g.ld)         # whole pixels of the wider buffers
    base = statistics.median(us['weighted_bce (existing pair)'])
    return {'views': {'N': N, 'HW': p.HW, 'C': p.C, 'ld_p': p.ld, 'ld_y': y.ld, 'ld_g': g.ld, 'slabs': int(L.load().pg_seg_loss_slabs(N, p.HW))},
            'MB_needed': round(need / 1e6, 1), 'MB_touched': round(touched / 1e6, 1),
            'us_per_pair': {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
            'ratio_to_existing_pair': {k: round(statistics.median(v) / base, 3) for k, v in us.items()},
            'TB_per_s_needed': {k: round(need / statistics.median(v) / 1e6, 2) for k, v in us.items()},
            'TB_per_s_touched': {k: round(touched / statistics.median(v) / 1e6, 2) for k, v in us.items()}}


out = {'metric': 'segmentation objectives: the two launches against the existing pair (us per pair, median of rounds; min..max), and the '
                 "cfg4-shape step with loss_type = 'ce+dice' against weighted_bce (ms per step)",
       'rounds': ROUNDS, 'reps_per_round': REPS,
       'cfg4_views': pair_times(CONFIGS['cfg4'], ['ce', 'focal', 'dice', 'ce+dice']),
       'cfg2_views': pair_times(CONFIGS['cfg2'], ['focal', 'dice', 'focal+dice'])}

if STEP:
    cfg = CONFIGS['cfg4']
    x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))

    def trainer(loss_type):
        torch.manual_seed(1234)
        G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
        D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False).to(dev)
        t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pgseg_'))
        t.loss_type, t.seg_alpha, t.gc_freeze, t.graph = loss_type, 200, True, 'auto'
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
    legs = {'weighted_bce': trainer('weighted_bce'), 'weighted_bce_again': trainer('weighted_bce'), 'ce+dice': trainer('ce+dice')}
    settle = 3 * (2 * pg.Trainer.TRIAL_STEPS + 2) + 4 + 12
    modes = {}
    for name, t in legs.items():
        run(t, settle)
        modes[name] = t.launch_mode
    ms = {k: [] for k in legs}
    for r in range(ROUNDS):
        for name, t in legs.items():
            run(t, 2)
            ms[name].append(run(t, STEPS))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out['cfg4_step'] = {'steps_per_round': STEPS, 'launch_mode': modes,
                        'ms_per_step': {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                        'weighted_bce_vs_again_ms': round(abs(med['weighted_bce'] - med['weighted_bce_again']), 3),
                        'ce+dice_minus_weighted_bce_ms': round(med['ce+dice'] - min(med['weighted_bce'], med['weighted_bce_again']), 3)}
print(json.dumps(out))
