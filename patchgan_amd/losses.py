"""Loss functions with the reference's names and argument order (patchgan/losses.py:5-39) for code that calls them
directly.  Inside ``Trainer.batch`` the losses and their gradients run as HIP kernels (engine.loss_value_and_grad);
these torch-op versions exist for API compatibility and work on any device torch supports."""
import torch
import torch.nn.functional as F
from torch import nn


def tversky(y_true, y_pred, beta, batch_mean=True):
    tp = torch.sum(y_true * y_pred, dim=(1, 2, 3))
    fn = torch.sum((1. - y_pred) * y_true, dim=(1, 2, 3))
    fp = torch.sum(y_pred * (1. - y_true), dim=(1, 2, 3))
    t = tp / (tp + beta * fn + (1. - beta) * fp)
    return torch.mean(1. - t) if batch_mean else (1. - t)


def fc_tversky(y_true, y_pred, beta, gamma=0.75, batch_mean=True):
    tp = torch.sum(y_true * y_pred, dim=(1, 2, 3))
    fn = torch.sum((1. - y_pred) * y_true, dim=(1, 2, 3))
    fp = torch.sum(y_pred * (1. - y_true), dim=(1, 2, 3))
    t = (tp + 1) / (tp + beta * fn + (1. - beta) * fp + 1)
    ft = 1 - t
    return torch.pow(torch.mean(ft), gamma) if batch_mean else torch.pow(ft, gamma)


def MAE_loss(y_true, y_pred):
    return torch.mean(torch.abs(y_true - y_pred))


bce_loss = nn.BCELoss()


# GAN objectives on a discriminator output d (Trainer.gan_mode; inside Trainer.batch they run as one HIP kernel, pg_gan_loss)
def lsgan_loss(d, target):
    """Least squares (Mao et al. 2017; pix2pix's gan_mode = lsgan): mean (d - target)^2, target a number or a tensor."""
    target = target if isinstance(target, torch.Tensor) else torch.full_like(d, float(target))
    return F.mse_loss(d, target)


def hinge_d_loss(d_real, d_fake):
    """The discriminator's hinge loss on logits (Miyato et al. 2018): (mean max(0, 1 - d_real) + mean max(0, 1 + d_fake)) / 2 -- the
    reference's / 2 on the discriminator loss stays."""
    return (torch.mean(F.relu(1. - d_real)) + torch.mean(F.relu(1. + d_fake))) / 2.


def hinge_g_loss(d_fake):
    """The generator's side of the hinge objective: -mean d_fake."""
    return -torch.mean(d_fake)


# Segmentation objectives on a generator output y_pred (probabilities, NCHW) against y_true (Trainer.loss_type = 'ce' | 'focal' | 'dice';
# inside Trainer.batch they run as two HIP kernels, pg_seg_loss_reduce / pg_seg_loss_value_grad).  Means over the batch, without seg_alpha.
def _clamped_log(x):
    return torch.clamp(torch.log(x), min=-100.)


def _ipow(x, k):
    """x^k by repeated multiplication (k a small non-negative integer; x^0 = 1 also at x = 0)."""
    out = torch.ones_like(x)
    for _ in range(k):
        out = out * x
    return out


def _per_class(class_weights, like):
    """class_weights (None or C numbers) as a [1, C, 1, 1] tensor beside `like` (NCHW), or None."""
    if class_weights is None:
        return None
    w = torch.as_tensor(class_weights, dtype=like.dtype, device=like.device).reshape(-1)
    if w.numel() != like.shape[1]:
        raise ValueError(f"class_weights has {w.numel()} entries for {like.shape[1]} channels")
    return w.view(1, -1, 1, 1)


def ce_loss(y_true, y_pred, class_weights=None):
    """Categorical cross-entropy on probabilities: the mean over pixels of -sum_c y log p, the log clamped at -100.  A pixel whose
    y_true is all zero (no listed label) adds nothing and still counts in the mean.
    class_weights (C numbers w_c): -sum_c w_c y log p, still divided by the number of pixels -- F.cross_entropy(logits, labels,
    weight=w, reduction='sum') / (N H W), not its weighted 'mean'."""
    n, _, h, w = y_pred.shape
    e = -y_true * _clamped_log(y_pred)
    cw = _per_class(class_weights, y_pred)
    if cw is not None:
        e = cw * e
    return torch.sum(e) / (n * h * w)


def focal_loss(y_true, y_pred, gamma=2, alpha=None, class_weights=None):
    """Focal loss (Lin et al. 2017), the binary form on every channel: mean -(a1 y (1-p)^gamma log p + a0 (1-y) p^gamma log(1-p)),
    gamma an integer in 0..8, a1 = alpha and a0 = 1 - alpha, or both 1 for alpha = None; gamma = 0 without alpha is
    F.binary_cross_entropy.  class_weights (C numbers w_c): channel c's elements times w_c, the mean still over all N C H W elements."""
    if isinstance(gamma, bool) or not isinstance(gamma, int) or not 0 <= gamma <= 8:
        raise ValueError(f"gamma must be an integer in 0 .. 8, not {gamma!r}")
    a1, a0 = (1., 1.) if alpha is None else (float(alpha), 1. - float(alpha))
    p, q = y_pred, 1. - y_pred
    lq = torch.clamp(torch.log1p(-p), min=-100.)
    e = -(a1 * y_true * _ipow(q, gamma) * _clamped_log(p) + a0 * (1. - y_true) * _ipow(p, gamma) * lq)
    cw = _per_class(class_weights, y_pred)
    if cw is not None:
        e = cw * e
    return torch.mean(e)


def dice_loss(y_true, y_pred, smooth=1.0, class_weights=None):
    """Soft Dice per sample and channel: the mean over (n, c) of 1 - (2 sum p y + smooth) / (sum p + sum y + smooth).
    class_weights (C numbers w_c): the mean over (n, c) of w_c (1 - D[n, c]), still over all N C pairs."""
    i = torch.sum(y_true * y_pred, dim=(2, 3))
    d = (2. * i + smooth) / (torch.sum(y_pred, dim=(2, 3)) + torch.sum(y_true, dim=(2, 3)) + smooth)
    t = 1. - d
    cw = _per_class(class_weights, y_pred)
    if cw is not None:
        t = cw.view(1, -1) * t
    return torch.mean(t)
