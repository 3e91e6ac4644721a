"""Segmentation metrics from counts kept on the device (beyond the reference, whose only quality signal is its six loss scalars).

Every score here -- IoU, Dice, precision, recall, pixel accuracy -- is a ratio of entries of a confusion matrix of integers.
engine.seg_confusion (pg_seg_confusion) adds one batch's counts to a small int64 device tensor beside the step's loss reductions;
the tensor is read once per pass (`SegCounts.read`), and `scores` turns it into numbers on the host in float64.

  C == 1 : prediction class = (p >= threshold), target class = (y >= 0.5); a 2 x 2 matrix, class 1 is the foreground
  C  > 1 : first maximum of the prediction against first maximum of the target; a pixel without a positive target channel (a
           one-hot mask over a label subset) is ignored and counted separately
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
        self.best[name] = {'epoch': int(epoch), 'score': score, 'scores': jsonable(score_dict)}
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
