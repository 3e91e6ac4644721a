"""Cost of Trainer.gan_mode = 'hinge' on Discriminator(final_act='none') at cfg2 (256x256, bs 16, nf = ndf = 64, fp32, graph = 'auto') on
one MI355X: ONE process, three trainers over the same generator configuration -- two default ones (their difference is the run-to-run
spread of this tool) and the hinge one -- alternated ROUNDS times, STEPS timed steps per leg and round (each trainer's launch mode is
decided and settled before the first timed round).  Then the loss launches on their own from HIP events on cfg2's 16 x 30 x 30 patch
map: the default step's six (pg_loss_reduce_parts + pg_loss_value_grad, three times) against the two pg_gan_loss calls.  Prints one
JSON line.  (The default step against the parent commit's: tools/ab.sh <parent tree> <this tree> <rounds>.)"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd import _lib as L
from patchgan_amd import engine as E
from bench import CONFIGS, make_inputs

ROUNDS, STEPS = int(os.environ.get('ROUNDS', '5')), int(os.environ.get('STEPS', '20'))
cfg = CONFIGS['cfg2']
dev = torch.device('cuda', 0)
x, y = (v.to(dev) for v in make_inputs(cfg['batch'], 0, cfg))


def trainer(gan_mode, final_act):
    torch.manual_seed(1234)
    G = pg.UNet(3, cfg['out_nc'], cfg['nf'], use_dropout=False, activation=cfg['activation'], final_act=cfg['final_act']).to(dev)
    D = pg.Discriminator(3 + cfg['out_nc'], cfg['ndf'], n_layers=cfg['n_layers'], norm=False, final_act=final_act).to(dev)
    t = pg.Trainer(G, D, tempfile.mkdtemp(prefix='pggan_'))
    t.loss_type, t.seg_alpha, t.gc_freeze, t.graph, t.gan_mode = cfg['loss_type'], 200, True, 'auto', gan_mode
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


legs = {'default': trainer('vanilla', 'sigmoid'), 'default_again': trainer('vanilla', 'sigmoid'), 'hinge': trainer('hinge', 'none')}
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
    return round(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps)), 4)


N = cfg['batch']
_, _, h, w = legs['default'].discriminator.engine.out_shape(N, 256, 256)
o2 = E.View(torch.rand(2 * N * h * w, device=dev) * 0.98 + 0.01, 0, 1, 2 * N, h, w, 1)
god = E.View.alloc(2 * N, h, w, 1, dev)
losses = torch.empty(4, device=dev)


def six_launches():
    E.loss_value_and_grad(o2.samples(N, N), None, 1.0, L.LOSS_BCE, 1.0, god.samples(N, N), losses, 1, N)
    E.loss_value_and_grad(o2.samples(0, N), None, 1.0, L.LOSS_BCE, 0.5, god.samples(0, N), losses, 2, N)
    E.loss_value_and_grad(o2.samples(N, N), None, 0.0, L.LOSS_BCE, 0.5, god.samples(N, N), losses, 3, N)


def two_launches():
    E.gan_loss([(o2.samples(N, N), L.GAN_HINGE_G, 1.0, 1.0, god.samples(N, N), 1)], losses, N)
    E.gan_loss([(o2.samples(0, N), L.GAN_HINGE_D, 1.0, 0.5, god.samples(0, N), 2), (o2.samples(N, N), L.GAN_HINGE_D, 0.0, 0.5, god.samples(N, N), 3)],
               losses, N)


kern = {'patch_map': [N, h, w], 'bce_six_launches_ms': events(six_launches), 'gan_loss_two_launches_ms': events(two_launches)}
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({'metric': "cfg2 training step, gan_mode = 'hinge' on a logit discriminator against the default step, ms per step "
                            '(median of rounds; min..max)',
                  'rounds': ROUNDS, 'steps_per_round': STEPS, 'launch_mode': modes,
                  'ms_per_step': {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  'default_vs_default_again_ms': round(abs(med['default'] - med['default_again']), 3),
                  'hinge_minus_default_ms': round(med['hinge'] - min(med['default'], med['default_again']), 3),
                  'loss_launches': kern}))
