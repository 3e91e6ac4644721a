"""f1 (BASELINE config 5): tiled inference throughput on one MI355X -- 1024x1024 image -> 25 overlapping 256x256 tiles
(overlap 0.9, infer.py:162) -> generator forward (eval) -> overlap-averaged mask.  Prints tiles/s, images/s, peak VRAM.
--tta hflip|flips|d4 and --window pyramid|hann time predict_image with test-time augmentation / a blend window (K variants of every
tile stream through the generator in passes of at most 64 tiles, as predict_image runs them)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import patchgan_amd as pg
from patchgan_amd.infer import predict_image
from patchgan_amd import engine as E

ap = argparse.ArgumentParser()
ap.add_argument('precision', nargs='?', default='fp32')      # tools/bench_infer.py bf16: bf16 kernels + bf16 activation storage
ap.add_argument('--tta', default=None, choices=['hflip', 'flips', 'd4'])
ap.add_argument('--window', default=None, choices=['pyramid', 'hann'])
args = ap.parse_args()
precision = args.precision
kw = {k: v for k, v in (('tta', args.tta), ('window', args.window)) if v is not None}      # none given: the call as it always was

torch.manual_seed(0)
g = pg.UNet(3, 1, 64, activation='leakyrelu', final_act='sigmoid').cuda().eval().set_precision(precision)
img = torch.rand(3, 1024, 1024).cuda()
reps = int(os.environ.get('REPS', '10'))
n = E.tiles_gather(img, 256, 0.9).N
for _ in range(2):
    predict_image(g, img, 256, 0.9, 0.5, **kw)
torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
t0 = time.perf_counter()
for _ in range(reps):
    m = predict_image(g, img, 256, 0.9, 0.5, **kw)    # includes the D2H copy of the 8 MB float64 mask
dt = (time.perf_counter() - t0) / reps
# device-side stages alone
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
ev[0].record()
tiles = E.tiles_gather(img, 256, 0.9, **({'tta': args.tta} if args.tta else {}))
ev[1].record()
pred = E.View.alloc(tiles.N, 256, 256, 1, 'cuda')
for t0 in range(0, tiles.N, 64):
    nt = min(64, tiles.N - t0)
    g.engine.forward(g.flat, tiles.samples(t0, nt), pred.samples(t0, nt), False, 0)
ev[2].record()
mask = E.tiles_blend(pred, (1024, 1024), 0.5, 0.9, **kw)
ev[3].record()
torch.cuda.synchronize()
what = ''.join(f', {k} {v}' for k, v in kw.items())
print(json.dumps({'metric': f'tiled inference, 1024x1024 -> 25 tiles of 256x256, UNet nf=64 {precision}{what}', 'tiles_per_s': round(n / dt, 1),
                  'images_per_s': round(1 / dt, 2), 'ms_per_image': round(dt * 1e3, 2), 'forwarded_tiles': tiles.N,
                  'gather_ms': round(ev[0].elapsed_time(ev[1]), 3), 'forward_ms': round(ev[1].elapsed_time(ev[2]), 3),
                  'blend_ms': round(ev[2].elapsed_time(ev[3]), 3),
                  'peak_vram_GiB': round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
