"""Segmentation metrics from counts kept on the device (beyond the reference, whose only quality signal is its six loss scalars).

Every score here -- IoU, Dice, precision, recall, pixel accuracy -- is a ratio of entries of a confusion matrix of integers.
engine.seg_confusion (pg_seg_confusion) adds one batch's counts to a small int64 device tensor beside the step's loss reductions;
the tensor is read once per pass (`SegCounts.read`), and `scores` turns it into numbers on the host in float64.

  C == 1 : prediction class = (p >= threshold), target class = (y >= 0.5); a 2 x 2 matrix, class 1 is the foreground
  C  > 1 : first maximum of the prediction against first maximum of the target; a pixel without a positive target channel (a
           one-hot mask over a label subset) is ignored and counted separately

Score curves (Trainer.metric_bins): engine.seg_hist (pg_seg_hist) adds, per channel and one-vs-rest label, a histogram of the prediction
over a power-of-two number of bins to a second int64 tensor (`SegHist`).  Its sums over the bins >= k are exactly the confusion counts at
threshold k / bins, so `curve` gives IoU / Dice / precision / recall at every threshold, average precision and the threshold with the
best IoU from one pass; `best_threshold` carries that threshold from best_metrics.json into patchgan_infer (`threshold: best`).
"""
import json
import math
import os

import numpy as np
import torch


class SegCounts:
    """The confusion counts of one pass: `t`, an int64 tensor of K*K + 1 words (K = 2 for one channel, else the channel count),
    [true class][predicted class] row-major and the number of ignored pixels in the last word.  engine.seg_confusion adds to it."""

    def __init__(self, C, device):
        if not 1 <= int(C) <= 32:
            raise ValueError(f"SegCounts: {C} channels (1 .. 32)")
        self.C = int(C)
        self.K = 2 if self.C == 1 else self.C
        self.t = torch.zeros(self.K * self.K + 1, dtype=torch.int64, device=device)

    def zero_(self):
        self.t.zero_()
        return self

    def read(self, dist=None):
        """(confusion np.int64 [K, K], ignored int).  Waits for the launches enqueued so far on the current stream.  Under a process
        group (dist = parallel.current() by default) the counts of all ranks are summed first: a COLLECTIVE, every rank calls it.  The
        tensor itself keeps this rank's counts, so reading twice counts nothing twice."""
        if dist is None:
            from .parallel import current
            dist = current()
        t = self.t
        if dist.on:
            t = t.clone()
            if t.is_cuda and dist.backend != 'nccl':
                t = t.cpu()
            dist.dist.all_reduce(t, op=dist.dist.ReduceOp.SUM)
        a = t.cpu().numpy().astype(np.int64, copy=True)          # (the device-to-host copy waits for the stream)
        K = self.K
        return a[:K * K].reshape(K, K), int(a[K * K])


def check_bins(bins):
    """`bins` as an int if it is a bin count pg_seg_hist takes (a power of two in 16..1024), else None."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        return None
    bins = int(bins)
    return bins if 16 <= bins <= 1024 and bins & (bins - 1) == 0 else None


class SegHist:
    """The prediction histograms of one pass, the twin of SegCounts: `t`, an int64 tensor of C*2*bins + 1 words, [channel][label][bin]
    row-major (label 1 = the pixel is of that class, one-vs-rest; bin b holds predictions in [b / bins, (b + 1) / bins), clamped to the
    first and last bin) and the number of ignored pixels in the last word.  engine.seg_hist adds to it."""

    def __init__(self, C, bins, device):
        if not 1 <= int(C) <= 32:
            raise ValueError(f"SegHist: {C} channels (1 .. 32)")
        if check_bins(bins) is None:
            raise ValueError(f"SegHist: {bins!r} bins (a power of two in 16 .. 1024)")
        if int(C) * int(bins) > 8192:
            raise ValueError(f"SegHist: {C} channels x {bins} bins (at most 8192 together)")
        self.C, self.bins = int(C), int(bins)
        self.t = torch.zeros(self.C * 2 * self.bins + 1, dtype=torch.int64, device=device)

    def zero_(self):
        self.t.zero_()
        return self

    def read(self, dist=None):
        """(hist np.int64 [C, 2, bins], ignored int).  As SegCounts.read: waits for the current stream, and under a process group sums
        the ranks' tables first -- a COLLECTIVE; the tensor keeps this rank's own counts."""
        if dist is None:
            from .parallel import current
            dist = current()
        t = self.t
        if dist.on:
            t = t.clone()
            if t.is_cuda and dist.backend != 'nccl':
                t = t.cpu()
            dist.dist.all_reduce(t, op=dist.dist.ReduceOp.SUM)
        a = t.cpu().numpy().astype(np.int64, copy=True)
        n = self.C * 2 * self.bins
        return a[:n].reshape(self.C, 2, self.bins), int(a[n])


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _nanmean(v):
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float('nan')


def scores(confusion):
    """Scores of a confusion matrix [true class][predicted class] (any integer or float array), in float64:
      iou, dice, precision, recall   arrays [K]: tp / (tp + fp + fn), 2 tp / (2 tp + fp + fn), tp / (tp + fp), tp / (tp + fn)
      pixel_acc                      trace / sum
      miou, mdice                    means of iou / dice over the classes that have one
      iou_fg, dice_fg                K == 2 only: class 1 (the foreground of a one-channel mask)
    A ratio with a zero denominator is nan (a class absent from prediction and target has no IoU and is left out of the means; the
    means are nan if every class is)."""
    c = np.asarray(confusion, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"scores: a square confusion matrix is needed, not shape {c.shape}")
    tp = np.diag(c)
    fp = c.sum(axis=0) - tp          # predicted as the class, of another class
    fn = c.sum(axis=1) - tp          # of the class, predicted as another
    out = {'iou': _ratio(tp, tp + fp + fn), 'dice': _ratio(2 * tp, 2 * tp + fp + fn), 'precision': _ratio(tp, tp + fp),
           'recall': _ratio(tp, tp + fn), 'pixel_acc': float(_ratio(tp.sum(), c.sum()))}
    out['miou'], out['mdice'] = _nanmean(out['iou']), _nanmean(out['dice'])
    if c.shape[0] == 2:
        out['iou_fg'], out['dice_fg'] = float(out['iou'][1]), float(out['dice'][1])
    return out


def report(confusion, ignored):
    """scores(confusion) plus the counts themselves: what Trainer.read_metrics / Trainer.evaluate return."""
    return dict(scores(confusion), confusion=confusion, ignored=int(ignored))


CURVE_ONLY = ('curve', 'hist')      # what read_metrics() returns per threshold / per bin: kept out of val_history and best_metrics.json


def curve(hist):
    """Scores at every threshold of a histogram table [C, 2, bins] ([channel][label][bin], SegHist.read), on the host in float64.
    Threshold k of `bins` is theta_k = k / bins, predicted positive means bin >= k, which is p >= theta_k exactly (a power-of-two bin
    count): the counts at k are those of pg_seg_confusion at metric_threshold = theta_k.
      'curve'         {'thresholds' [bins], 'tp', 'fp', 'fn', 'tn' (int64 [C, bins]), 'precision', 'recall', 'iou', 'dice' ([C, bins])}
      ap              [C]: sum over k of (recall[k] - recall[k+1]) * precision[k], recall[bins] := 0; a term without a precision (nothing
                      predicted at k: its recall step is 0 as well) counts as 0; nan for a class without a positive pixel
      best_threshold  [C]: theta_k of the SMALLEST k >= 1 with the largest IoU of the class (k = 0 is left out: a threshold of 0 turns
                      thresholding off in patchgan_infer); nan if the class has no IoU at any k.  Dice is monotone in IoU: the same k
                      maximises it.
      best_iou, best_dice   [C]: the values at that k
      mean_ap, best_miou    means over the classes that have one (nan if none has)"""
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[1] != 2:
        raise ValueError(f"curve: a histogram table [C, 2, bins] is needed, not shape {h.shape}")
    h = h.astype(np.int64)
    C, _, bins = h.shape
    tp = np.cumsum(h[:, 1, ::-1], axis=1)[:, ::-1]          # sum over b >= k
    fp = np.cumsum(h[:, 0, ::-1], axis=1)[:, ::-1]
    pos, neg = h[:, 1].sum(axis=1), h[:, 0].sum(axis=1)
    fn, tn = pos[:, None] - tp, neg[:, None] - fp
    precision, recall = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    iou, dice = _ratio(tp, tp + fp + fn), _ratio(2 * tp, 2 * tp + fp + fn)
    ap = np.full(C, np.nan)
    best_t, best_iou, best_dice = np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan)
    for c in range(C):
        if pos[c] > 0:
            step = recall[c] - np.append(recall[c, 1:], 0.0)
            ap[c] = float(np.sum(step * np.where(np.isnan(precision[c]), 0.0, precision[c])))
        v = iou[c, 1:]
        ok = ~np.isnan(v)
        if ok.any():
            k = 1 + int(np.argmax(np.where(ok, v, -np.inf)))          # (argmax: the first of equal maxima)
            best_t[c], best_iou[c], best_dice[c] = k / bins, iou[c, k], dice[c, k]
    return {'curve': {'thresholds': np.arange(bins, dtype=np.float64) / bins, 'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn,
                      'precision': precision, 'recall': recall, 'iou': iou, 'dice': dice},
            'ap': ap, 'best_threshold': best_t, 'best_iou': best_iou, 'best_dice': best_dice,
            'mean_ap': _nanmean(ap), 'best_miou': _nanmean(best_iou)}


def report_curve(hist):
    """curve(hist) plus the table itself: what Trainer.read_metrics / Trainer.evaluate add with metric_bins."""
    return dict(curve(hist), hist=hist)


def best_threshold(checkpoint_path, out_channels):
    """The threshold `infer_params.threshold: best` stands for: best_threshold of the model stored as `checkpoint_path`, read from the
    best_metrics.json beside it (written by train() with save_best and metric_bins).  Only best_generator.pth (entry 'generator') and
    best_generator_ema.pth ('generator_ema') have one -- a threshold measured for another epoch's weights is not the best for these --
    and only a generator with one output channel is thresholded by a single number.  ValueError names what is missing."""
    name = os.path.basename(str(checkpoint_path))
    entry = {'best_generator.pth': 'generator', 'best_generator_ema.pth': 'generator_ema'}.get(name)
    if entry is None:
        raise ValueError(f"threshold: best needs checkpoint_paths.generator to be a best_generator.pth or best_generator_ema.pth "
                         f"written by save_best, not {name!r} (the stored threshold was measured for those weights only)")
    if int(out_channels) != 1:
        raise ValueError(f"threshold: best needs a generator with one output channel, not {out_channels} "
                         f"(several channels are thresholded and then compared: no single best threshold)")
    path = os.path.join(os.path.dirname(str(checkpoint_path)), BestTracker.FILE)
    if not os.path.exists(path):
        raise ValueError(f"threshold: best needs {path} (train with save_best and metric_bins)")
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d.get(entry), dict):
        raise ValueError(f"threshold: best: {path} has no entry {entry!r} for {name}")
    value = (d[entry].get('scores') or {}).get('best_threshold')
    if isinstance(value, (list, tuple)):
        value = value[0] if len(value) == 1 else None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value):
        raise ValueError(f"threshold: best: entry {entry!r} of {path} holds no best_threshold (train with metric_bins set)")
    return float(value)


def jsonable(d):
    """A score dict with arrays as lists and nan as None (strict JSON has no nan)."""
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, np.ndarray):
            return [conv(x) for x in v.tolist()]
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return None if math.isnan(v) else float(v)
        if isinstance(v, np.integer):
            return int(v)
        return v
    return conv(d)


class BestTracker:
    """The best-so-far rule of Trainer.save_best: per tracked model ('generator', 'generator_ema') the epoch, score and score dict
    of its best validation so far.  A score wins only if it is STRICTLY greater than the stored one; nan never wins.  Stored as
    best_metrics.json beside the checkpoints and read back on resume, so a resumed run does not replace a better model by a worse one."""

    FILE = 'best_metrics.json'

    def __init__(self, metric, best=None):
        if metric not in ('miou', 'mdice'):
            raise ValueError(f"save_best must be None, 'miou' or 'mdice', not {metric!r}")
        self.metric = metric
        self.best = dict(best or {})

    def update(self, name, epoch, score_dict):
        """True (and remembered) if score_dict[metric] beats the best of `name` so far."""
        score = float(score_dict[self.metric])
        have = self.best.get(name)
        if math.isnan(score) or (have is not None and have['score'] is not None and not score > have['score']):
            return False
        # (the per-threshold arrays and the histogram of metric_bins stay out of the file; best_threshold and the other values stay in)
        kept = {k: v for k, v in score_dict.items() if k not in CURVE_ONLY}
        self.best[name] = {'epoch': int(epoch), 'score': score, 'scores': jsonable(kept)}
        return True

    def to_dict(self):
        return dict({'metric': self.metric}, **self.best)

    def save(self, folder):
        path = os.path.join(folder, self.FILE)
        with open(path + '.tmp', 'w') as f:
            json.dump(self.to_dict(), f, indent=1)
        os.replace(path + '.tmp', path)
        return path

    @classmethod
    def load(cls, folder):
        """The tracker stored in `folder`, or None without a (readable) best_metrics.json."""
        path = os.path.join(folder, cls.FILE)
        if not os.path.exists(path):
            return None
        with open(path) as f:
            d = json.load(f)
        return cls(d.pop('metric'), d)
