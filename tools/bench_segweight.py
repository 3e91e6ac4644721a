"""Cost of per-class weights (Trainer.class_weights; pg_seg_loss_value_grad_w, pg_seg_label_count of segloss.hip) on one MI355X, in ONE
process, from HIP events, on the views of tools/bench_segloss.py: a cfg4 step's (8 x 512 x 512, 4 classes, prediction and target 3
floats into 8-float pixels, the gradient dense) and a cfg2 step's (16 x 256 x 256, one channel, 3 floats into 4-float pixels).
  1. pg_seg_loss_reduce + pg_seg_loss_value_grad_w against pg_seg_loss_reduce + pg_seg_loss_value_grad -- the parent's code -- and that
     pair a second time (the difference of the two unweighted legs is the spread of this tool), alternated ROUNDS times, median of REPS
     calls per leg and round, for every objective the view takes.
  2. pg_seg_label_count against pg_seg_confusion on the same target (the confusion pass reads the prediction as well).
Prints one JSON line."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from patchgan_amd import engine as E
from bench import CONFIGS

ROUNDS, REPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('REPS', '30'))
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
    """(p, y, g) as a step of this configuration lays them out (tools/bench_segloss.py: views)."""
    N, S, C = cfg['batch'], cfg['size'], cfg['out_nc']
    ld = -(-(3 + C) // 4) * 4
    gen = torch.Generator(device=dev).manual_seed(5)
    din = torch.rand(2 * N * S * S * ld, device=dev, generator=gen) * 0.98 + 0.01
    real = E.View(din, 0, ld, N, S, S, ld).channels(3, C)
    fake = E.View(din, N * S * S * ld, ld, N, S, S, ld).channels(3, C)
    y = (torch.rand(N, C, S, S, device=dev, generator=gen) > 0.7).float()
    din[:N * S * S * ld].view(N, S, S, ld)[..., 3:3 + C] = y.permute(0, 2, 3, 1)
    return fake, real, E.View.alloc(N, S, S, C, dev)


def summary(v):
    return [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]


def pair_times(cfg, names):
    p, y, g = views(cfg)
    N, C = p.N, p.C
    loss = torch.empty(1, device=dev)
    final_act = 'softmax' if C > 1 else 'sigmoid'
    weights = [0.1, 37.5, 0.5, 1.0][:C] if C > 1 else [2.0]
    out = {}
    for name in names:
        plain = E.check_seg_loss(name, final_act, C)
        weighted = E.check_seg_loss(name, final_act, C, class_weights=weights, device=dev)
        legs = {'unweighted': lambda: E.seg_loss_finish(E.seg_loss_begin(p, y, plain), 200.0, g, loss, 0, N),
                'unweighted_again': lambda: E.seg_loss_finish(E.seg_loss_begin(p, y, plain), 200.0, g, loss, 0, N),
                'weighted': lambda: E.seg_loss_finish(E.seg_loss_begin(p, y, weighted), 200.0, g, loss, 0, N)}
        us = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, fn in legs.items():
                us[k].append(events(fn, REPS) * 1e3)
        med = {k: statistics.median(v) for k, v in us.items()}
        out[name] = {'us_per_pair': {k: summary(v) for k, v in us.items()},
                     'spread_of_two_unweighted_legs_us': round(abs(med['unweighted'] - med['unweighted_again']), 2),
                     'weighted_minus_unweighted_us': round(med['weighted'] - min(med['unweighted'], med['unweighted_again']), 2)}
    # the label count against the confusion counts on the same target
    K = 2 if C == 1 else C
    conf = torch.zeros(K * K + 1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(C + 2, dtype=torch.int64, device=dev)
    legs = {'pg_seg_confusion': lambda: E.seg_confusion(p, y, 0.5, conf), 'pg_seg_label_count': lambda: E.seg_label_count(y, cnt)}
    us = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            us[k].append(events(fn, REPS) * 1e3)
    touched = p.npix * y.ld * 4
    return {'views': {'N': N, 'HW': p.HW, 'C': C, 'ld_p': p.ld, 'ld_y': y.ld, 'ld_g': g.ld}, 'weights': weights, 'pairs': out,
            'counts_us': {k: summary(v) for k, v in us.items()},
            'label_count_TB_per_s_touched': round(touched / statistics.median(us['pg_seg_label_count']) / 1e6, 2),
            'label_count_MB_touched': round(touched / 1e6, 1)}


print(json.dumps({'metric': 'per-class weights: the weighted pair against the unweighted pair on the same views (us per pair: median of rounds, '
                            'min, max), and pg_seg_label_count against pg_seg_confusion (us per launch)',
                  'rounds': ROUNDS, 'reps_per_round': REPS,
                  'cfg4_views': pair_times(CONFIGS['cfg4'], ['ce', 'focal', 'dice', 'ce+dice', 'ce+focal+dice']),
                  'cfg2_views': pair_times(CONFIGS['cfg2'], ['focal', 'dice', 'focal+dice'])}))
