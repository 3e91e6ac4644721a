"""Cost of the segmentation metrics (Trainer.metrics) on the GPU, three measurements (EXPERIMENTS.md):

  kernel   pg_seg_confusion against pg_loss_reduce_parts on the same views in the same run: HIP events around 50 back-to-back
           launches, median of 9 windows -- cfg2's views (16 x 256^2, C = 1, a slice of ld = 4) and cfg4's (8 x 512^2, C = 4, a slice
           of ld = 7).  Both read N*HW*2C*4 bytes.
  hist     pg_seg_hist (256 bins) against pg_seg_confusion on the same views in the same run, alternating windows: cfg2's and cfg4's
           views, once with uniform random predictions and once with saturated ones (every value 0 or 1)
  pass     an evaluation step at cfg2 with metrics = True against None, alternating blocks of 20 steps; evaluate() per batch; the
           same with metric_bins = 256 against None (metrics on in both)
  host     the host-side route for one cfg2 batch: to_nchw().cpu() + the NumPy confusion matrix, against the kernel

    python tools/metrics_bench.py [kernel] [hist] [pass] [host]
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import patchgan_amd as pg
from patchgan_amd import _lib as L
from patchgan_amd import engine as E

DEV = torch.device('cuda', 0)


def timed(fn, launches=50, windows=9):
    """Median over `windows` of the time per launch of `launches` back-to-back calls, in microseconds."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return statistics.median(out), min(out), max(out)


def views(N, H, C, ld, off):
    g = torch.Generator(device='cuda').manual_seed(1)
    pbuf = torch.rand(N * H * H * ld, device=DEV, generator=g).clamp_(1e-3, 1 - 1e-3)
    ybuf = (torch.rand(N * H * H * ld, device=DEV, generator=g) > 0.7).float()
    return E.View(pbuf, off, ld, N, H, H, C), E.View(ybuf, off, ld, N, H, H, C)


def kernel():
    lib = L.load()
    res = {}
    for name, (N, H, C, ld, off) in {'cfg2': (16, 256, 1, 4, 3), 'cfg4': (8, 512, 4, 7, 3), 'cfg4_ld4': (8, 512, 4, 4, 0)}.items():
        p, y = views(N, H, C, ld, off)
        K = 2 if C == 1 else C
        counts = torch.zeros(K * K + 1, dtype=torch.int64, device=DEV)
        S = torch.empty(int(lib.pg_loss_reduce_doubles(N, H * H, C)), dtype=torch.float64, device=DEV)

        def conf():
            L.check(lib.pg_seg_confusion(p.ptr(), p.ld, y.ptr(), y.ld, N, H * H, C, 0.5, counts.data_ptr(), E._stream()), 'pg_seg_confusion')

        def loss():
            assert lib.pg_loss_reduce_parts(p.ptr(), p.ld, y.ptr(), y.ld, 0.0, N, H * H, C, S.data_ptr(), E._stream()) >= 1
        mb = N * H * H * 2 * C * 4 / 1e6
        tc, tl = timed(conf), timed(loss)
        res[name] = {'MB': mb, 'seg_confusion_us': tc, 'loss_reduce_parts_us': tl, 'seg_confusion_TBps': mb / tc[0], 'loss_reduce_parts_TBps': mb / tl[0]}
    return res


def timed_pair(fa, fb, launches=50, windows=9):
    """timed() of two launches in ALTERNATING windows (a, b, a, b, ...): clock and cache state drift hits both alike."""
    for _ in range(5):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(windows):
        for fn, dst in ((fa, out[0]), (fb, out[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            dst.append(a.elapsed_time(b) * 1e3 / launches)
    return tuple((statistics.median(v), min(v), max(v)) for v in out)


def hist(bins=256):
    lib = L.load()
    res = {}
    for name, (N, H, C, ld, off) in {'cfg2': (16, 256, 1, 4, 3), 'cfg4': (8, 512, 4, 7, 3)}.items():
        for kind in ('uniform', 'saturated'):
            p, y = views(N, H, C, ld, off)
            if kind == 'saturated':
                p.t.copy_((p.t > 0.5).float())
            K = 2 if C == 1 else C
            counts = torch.zeros(K * K + 1, dtype=torch.int64, device=DEV)
            table = torch.zeros(C * 2 * bins + 1, dtype=torch.int64, device=DEV)

            def conf():
                L.check(lib.pg_seg_confusion(p.ptr(), p.ld, y.ptr(), y.ld, N, H * H, C, 0.5, counts.data_ptr(), E._stream()), 'pg_seg_confusion')

            def hst():
                L.check(lib.pg_seg_hist(p.ptr(), p.ld, y.ptr(), y.ld, N, H * H, C, bins, table.data_ptr(), E._stream()), 'pg_seg_hist')
            th, tc = timed_pair(hst, conf)
            res[f'{name}_{kind}'] = {'MB': N * H * H * 2 * C * 4 / 1e6, 'bins': bins, 'seg_hist_us': th, 'seg_confusion_us': tc,
                                     'ratio': th[0] / tc[0]}
    return res


def cfg2_trainer():
    torch.manual_seed(1)
    g = pg.UNet(3, 1, 64, use_dropout=False, activation='leakyrelu', final_act='sigmoid').to(DEV)
    d = pg.Discriminator(4, 64, n_layers=3).to(DEV)
    t = pg.Trainer(g, d, tempfile.mkdtemp())
    g.eval()
    d.eval()
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(16, 3, 256, 256, generator=gen).to(DEV)
    y = (torch.rand(16, 1, 256, 256, generator=gen) > 0.7).float().to(DEV)
    return t, x, y


def block(fn, steps=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def pass_cost():
    t, x, y = cfg2_trainer()
    res = {}
    for two in (False, True):
        t.two_streams = two
        ms = {None: [], True: []}
        for on in (None, True):          # warm both kinds
            t.metrics = on
            block(lambda: t.batch(x, y, train=False), 5)
        for _ in range(5):
            for on in (None, True):
                t.metrics = on
                ms[on].append(block(lambda: t.batch(x, y, train=False)))
        res['eval_step_two_streams' if two else 'eval_step_one_stream'] = {
            'off_ms': [round(v, 4) for v in ms[None]], 'on_ms': [round(v, 4) for v in ms[True]],
            'off_median_ms': statistics.median(ms[None]), 'on_median_ms': statistics.median(ms[True])}
    t.metrics = True
    for two in (False, True):          # the histogram launch: metric_bins = 256 against None, the confusion counts on in both
        t.two_streams = two
        ms = {None: [], 256: []}
        for bins in (None, 256):
            t.metric_bins = bins
            block(lambda: t.batch(x, y, train=False), 5)
        for _ in range(5):
            for bins in (None, 256):
                t.metric_bins = bins
                ms[bins].append(block(lambda: t.batch(x, y, train=False)))
        res['eval_step_bins_two_streams' if two else 'eval_step_bins_one_stream'] = {
            'off_ms': [round(v, 4) for v in ms[None]], 'on_ms': [round(v, 4) for v in ms[256]],
            'off_median_ms': statistics.median(ms[None]), 'on_median_ms': statistics.median(ms[256])}
    t.metric_bins = None
    data = [(x, y)] * 20
    t.evaluate(data[:5])
    ev = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.evaluate(data)
        ev.append((time.perf_counter() - t0) * 1e3 / len(data))
    res['evaluate_per_batch_ms'] = [round(v, 4) for v in ev]
    return res


def host():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from metrics_util import confusion_ref
    t, x, y = cfg2_trainer()
    t.metrics = True
    t.batch(x, y, train=False)
    gen, yh = t._last_gen, y.cpu().numpy()
    yv = E.View(y.permute(0, 2, 3, 1).contiguous().reshape(-1), 0, 1, 16, 256, 256, 1)
    counts = torch.zeros(5, dtype=torch.int64, device=DEV)
    out = {'copy_ms': [], 'numpy_ms': [], 'kernel_and_read_ms': []}
    for _ in range(5):          # the host-side route: layout pass + synchronising copy, then NumPy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ph = gen.to_nchw().cpu().numpy()
        t1 = time.perf_counter()
        ref = confusion_ref(ph, yh, 0.5)
        t2 = time.perf_counter()
        out['copy_ms'].append(round((t1 - t0) * 1e3, 3))
        out['numpy_ms'].append(round((t2 - t1) * 1e3, 3))
    for _ in range(6):          # the device route WITH its read (a pass reads once, not per batch); the first round warms up
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        counts.zero_()
        E.seg_confusion(gen, yv, 0.5, counts)
        got = counts.cpu().numpy()
        t3 = time.perf_counter()
        assert np.array_equal(got[:4].reshape(2, 2), ref[0])
        out['kernel_and_read_ms'].append(round((t3 - t2) * 1e3, 3))
    out['kernel_and_read_ms'] = out['kernel_and_read_ms'][1:]
    return out


if __name__ == '__main__':
    which = sys.argv[1:] or ['kernel', 'hist', 'pass', 'host']
    fns = {'kernel': kernel, 'hist': hist, 'pass': pass_cost, 'host': host}
    for w in which:
        print(json.dumps({w: fns[w]()}), flush=True)
