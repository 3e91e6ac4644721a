"""Trainer with the reference's surface (patchgan/trainer.py:16-321): ``batch`` (one generator + one
discriminator update), ``train`` (epoch driver, Adam, LR schedule, checkpoints), ``save`` / ``load`` /
``load_last_checkpoint`` -- the G+D step hand-scheduled on the HIP engines instead of autograd.

Per-step schedule (reference trainer.py:50-115):
   x, y -> NHWC slices of ONE discriminator-input buffer din[2N] (real half = x|y, fake half = x|G(x)):
   G fwd (dec6 writes straight into the fake half) -> D fwd(fake) -> seg loss + BCE(D(fake),1) ->
   dgrad through D (its weight grads are skipped: the reference zeroes them at trainer.py:93-94) ->
   G bwd -> Adam(G) -> D fwd over din[2N] (real and detached fake in one batch) -> BCE halves -> D bwd -> Adam(D) ->
   one device->host copy of the loss scalars.
   Where the planner allows it (SHARE_D_FAKE, DiscriminatorEngine.halves_ok) the two D forwards are two N-sample half passes that fill
   ONE 2N context: D fwd(fake) is its fake half, the later pass only adds the real half -- D(x | G(x)) is computed once.
   Under data parallelism: G's gradient buckets are all-reduced asynchronously from inside G bwd and Adam(G) moves behind
   the D backward; D's gradient is all-reduced asynchronously and Adam(D) moves behind the next step's G forward (flush()).
   On two streams (a device-bound kind of step; engine.Exec) the same launches are spread over two in-order chains: the weight
   gradients of each backward pass, the D forward over din[2N] (enqueued as soon as G's output exists) and the whole D backward pass +
   Adam(D) (which then run under the NEXT step's G forward) go to the second stream; flush() joins before D's weights are read.
   How a kind of step is launched -- one stream, two streams, a replay of the captured hipGraph -- is measured, not guessed
   (_launch_mode: a tournament over the candidates the settings allow).
   With Discriminator(spectral_norm=True) every D pass above reads ONE normalised copy of D's weights, made once per call right after
   flush() (one power iteration while D is in training mode), and Adam(D) is preceded by the map of the flat gradient back to the stored
   weights (_adam_step) -- one iteration per step, where torch's hook on a wrapped reference D would iterate on each of its three calls.
   With Trainer.diffaug set, a training step's D passes read T(din), a per-sample flip / translation / cutout of the input buffer
   made by two moves (the real half ahead of the generator forward, the fake half behind it), and the gradient returns to G through
   the adjoint move; the draws come from a device-resident counter-based stream, so every launch mode sees the same tables.
   With Trainer.gan_mode / real_label set, or a Discriminator(final_act='none'), the three BCE terms above become the terms of the chosen
   objective (least squares, hinge, BCE with logits), evaluated by pg_gan_loss: one launch for the generator step's term, one for the
   discriminator step's two.
   With Trainer.loss_type = 'ce' | 'focal' | 'dice' or a sum of them, the segmentation loss's two launches -- one in front of D
   fwd(fake), one behind it -- are pg_seg_loss_reduce and pg_seg_loss_value_grad instead of the reference objectives' pair.

Data parallelism: one process per GPU (torch.distributed, backend "nccl" = RCCL).  InstanceNorm is per sample,
so the only exchanges are the SUM all-reduce of the flat gradient buffers and of two loss-normalisation terms
(focal-Tversky's batch mean and weighted-BCE's sum(y) are non-linear in the batch).  Gradient seeds are scaled
by the GLOBAL batch so the summed gradient equals the single-process large-batch gradient.
"""
import glob
import os
import time
from collections import defaultdict, namedtuple

import numpy as np
import torch
import tqdm

from . import _lib as L
from . import engine as E
from .metrics import CURVE_ONLY, BestTracker, SegCounts, SegHist, check_bins, report, report_curve
from .parallel import current as _dist, GradReducer

device = 'cuda' if torch.cuda.is_available() else 'cpu'

_LOSS_MODES = {'tversky': L.LOSS_TVERSKY, 'weighted_bce': L.LOSS_WBCE, 'MAE': L.LOSS_MAE}
EARLY_D_FWD = E._exp_env('PATCHGAN_EARLY_D_FWD') != '0'      # two-stream step: the discriminator step's forward under the generator step (A/B switch)
ADAM_G_BESIDE = E._exp_env('PATCHGAN_ADAM_G_BESIDE') != '0'      # ... and G's Adam update behind that fork (A/B switch)
# (under data parallelism too -- with the runtime's default of 4 hardware queues it measured SLOWER there, 9.06 vs 8.89 ms with a one-rank
#  RCCL group: the compute stream shared a hardware queue with a stream waiting for the deferred pass; patchgan_amd/__init__.py asks
#  for 8 queues: 8.51)
DEFER_D_BWD_DP = E._exp_env('PATCHGAN_DEFER_D_BWD_DP') != '0'
# D(x | G(x)) once per step: the generator step's pass over the fake batch and the fake half of the discriminator step's 2N pass read the
# same bytes with the same weights -- run as two half passes that fill ONE 2N context (engine.DiscriminatorEngine.forward_part) where the
# planner says the halves compute what the whole computes (halves_ok); off = the reference's three passes (A/B switch, tests)
SHARE_D_FAKE = E._exp_env('PATCHGAN_SHARE_D_FAKE') != '0'
DEFER_D_BWD = E._exp_env('PATCHGAN_DEFER_D_BWD') != '0'      # two-stream step: the discriminator's backward pass + Adam(D) under the NEXT step's generator forward (A/B switch)

# One network's side of the optimizer (Trainer._opt): i = 0 (generator) | 1 (discriminator) indexes the per-network pairs, t is the
# Adam step count, scal the network's slice of a captured step's device scalars
_Opt = namedtuple('_Opt', 'i net m v t lr betas weight_decay max_norm ema ema_decay acc scal')


_GC_FREEZES = 0


def _settle_gc(step):
    """Keep CPython's cyclic collector out of the step loop's way -- OPT-IN (Trainer.gc_freeze; bench.py and the patchgan_train
    entry point set it, a program that embeds Trainer is left alone: gc.freeze() is process-global and would move the host
    application's own objects to the permanent generation as well).  A full (generation-2) collection walks every live container
    object of the process -- ~0.5 M after `import torch` -- and takes 40-70 ms here: four to fifteen G+D steps of GPU time during
    which the host enqueues nothing (measured: one such pause inside a 20-step bench window moved bf16 cfg2 from 4.3 to 6.2 ms per
    step).  After the first and after the third training step of the process -- by then the engines' kernel plans, workspaces and
    weight caches exist -- collect once and move everything alive into the permanent generation (gc.freeze()): later collections
    only look at what the steps themselves create.  Trainer.train() undoes it (gc.unfreeze()) when it returns.
    PATCHGAN_GC_FREEZE=0 switches it off everywhere."""
    global _GC_FREEZES
    if _GC_FREEZES >= 2 or step not in (1, 3) or os.environ.get('PATCHGAN_GC_FREEZE', '1') == '0':
        return
    import gc
    gc.collect()
    gc.freeze()
    _GC_FREEZES += 1


def _unsettle_gc():
    """Hand the objects frozen by _settle_gc back to the collector (end of Trainer.train)."""
    global _GC_FREEZES
    if _GC_FREEZES:
        import gc
        gc.unfreeze()
        _GC_FREEZES = 0


class StepLosses(dict):
    """The six loss scalars of one step (reference trainer.py:108-115 returns them as a dict of floats).  A dict whose content
    arrives with the step's device-to-host copy: Trainer.batch returns as soon as the step is enqueued and the FIRST access waits
    for that copy, so a caller that reads the values later (the epoch loop reads step i after enqueuing step i + 1, bench.py after
    its timed region) does not drain the GPU between steps (the end-of-step wait left it idle for 0.12-0.15 ms: the host needs
    that long to get the next step's first kernels out)."""

    KEYS = ('gen', 'gen_loss', 'gdisc', 'discr', 'discf', 'disc')

    def __init__(self, host, event):
        super().__init__()
        self._host, self._event = host, event

    def _fill(self):
        if self._host is not None:
            self._event.synchronize()
            v = self._host.numpy()
            seg, gdisc = np.float32(v[0]), np.float32(v[1])
            loss_real, loss_fake = np.float32(v[2]) * np.float32(2), np.float32(v[3]) * np.float32(2)
            gen_loss = seg + gdisc
            disc_loss = (loss_fake + loss_real) / np.float32(2)
            vals = [float(gen_loss), float(gen_loss), float(gdisc), float(loss_real), float(loss_fake), float(disc_loss)]
            self._host = self._event = None
            dict.update(self, zip(self.KEYS, vals))
        return self

    def __getitem__(self, k):
        return dict.__getitem__(self._fill(), k)

    def __iter__(self):
        return dict.__iter__(self._fill())

    def __len__(self):
        return dict.__len__(self._fill())

    def __contains__(self, k):
        return dict.__contains__(self._fill(), k)

    def __repr__(self):
        return dict.__repr__(self._fill())

    def __eq__(self, other):
        if isinstance(other, StepLosses):
            other._fill()
        return dict.__eq__(self._fill(), other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def keys(self):
        return dict.keys(self._fill())

    def values(self):
        return dict.values(self._fill())

    def items(self):
        return dict.items(self._fill())

    def get(self, k, default=None):
        return dict.get(self._fill(), k, default)

    def copy(self):
        return dict(self._fill())

    def __reduce__(self):
        return (dict, (dict(self._fill()),))


def weights_init(net, init_type='normal', scaling=0.02):
    """The reference's ``weights_init`` defines an inner function and never applies it (trainer.py:327-343):
    a no-op, so torch's default initialisation stays.  Kept as a no-op for parity."""
    return None


class Trainer:
    seg_alpha = 200
    loss_type = 'tversky'
    tversky_beta = 0.75
    tversky_gamma = 0.75

    # Exponential moving average of the GENERATOR's weights (opt-in, beyond the reference): None = off -- no buffer, the same launches.
    # A float in [0, 1): from the next setup_optimizers() on (train() calls it) a second flat buffer follows the weights inside G's
    # Adam kernel, ema += (w_new - ema) * (1 - ema_decay) (pg_adam_ema_step), and `ema_generator` is a UNet in eval mode whose
    # parameters are views of that buffer: what one checkpoints and predicts with.  Not optimizer state: a later setup_optimizers() /
    # train() keeps it, reset_ema() restarts it from the live weights.  Every rank of a data-parallel job applies the same update to
    # the same all-reduced gradient, so the averages agree without a collective.
    ema_decay = None

    # Gradient-norm clipping and non-finite step skip (opt-in, beyond the reference, whose users put torch.nn.utils.clip_grad_norm_
    # between backward() and optimizer.step()): None = off -- no buffer, the same launches.  A positive float (float('inf') = monitor
    # only) for both networks, or a pair (gen_max_norm, disc_max_norm) whose members may be None.  In front of a network's Adam launch
    # -- in every launch mode, on whatever stream that launch is on, under data parallelism after the all-reduce -- pg_grad_norm takes
    # the 2-norm of its whole flat gradient (fp64, fixed order: the same bits in every mode and on every rank) and leaves
    # coef = min(1, max_norm / (norm + 1e-6)) in a device status block; pg_adam_clip_step applies g * coef inside the fused Adam pass.
    # A gradient with a NaN or an inf in it SKIPS the step: weights, moments and the weight average keep their bits.  The host never
    # reads the device for this, so Adam's step count advances on a skipped step as well: the bias correction of the following steps
    # is one step ahead (harmless after a few hundred steps), and the running statistics of nn.BatchNorm2d layers, which the FORWARD
    # pass updates, are not protected.  read_grad_stats() / reset_grad_stats(); train() reads once per epoch into `grad_history`.
    clip_grad_norm = None

    # Differentiable augmentation of what the discriminator sees (opt-in, beyond the reference; Zhao et al. 2020): None = off -- no buffer,
    # the same launches, the same kind key, the same bits.  A comma-separated string or a sequence out of 'flip', 'translation', 'cutout'
    # (engine.diffaug_policy; applied in that order): in a TRAINING step every discriminator pass -- the generator step's D(x | G(x)), the
    # discriminator step's real and fake halves, and both backward passes -- reads T(din) instead of din, T a per-sample map of pixels
    # (horizontal flip, translation by up to 1/8 of the extent with zero padding, a zeroed box of half the extent; pg_diffaug_fwd),
    # and the gradient returns to the generator through its exact adjoint (pg_diffaug_bwd).  Real sample i and fake sample i take the SAME
    # row of the step's parameter table (the condition image stays consistent), drawn once per call on the device by pg_diffaug_params
    # from (diffaug_seed, a step count kept in a device word, the GLOBAL sample index): a captured step replays with fresh draws, and
    # the ranks of a data-parallel job draw what the single process draws for the large batch.  The generator's output, the segmentation
    # loss, the metrics and evaluation steps stay on the un-augmented tensors; evaluation steps do not advance the count.
    # read_diffaug_params() returns the last step's table.  The count is checkpointed with save_optimizer (as is the step number
    # dropout's seeds derive from); without it a resumed run starts the stream again.
    diffaug = None
    diffaug_seed = 0         # a stream of its own, independent of dropout's

    # The adversarial objective (opt-in, beyond the reference, whose objective is nn.BCELoss on a sigmoid patch map): 'vanilla' with
    # real_label = 1 on a sigmoid discriminator = off -- the same launches, buffers, bits and kind key.  d_f = D(T(x | G(x))),
    # d_r = D(T(x | y)), means over all values of a term, r = real_label (the discriminator's real term only: one-sided smoothing),
    # disc = (real + fake) / 2 and gen = seg + gdisc as in the reference:
    #   'vanilla'   sigmoid D: BCE(d_f, 1) | BCE(d_r, r), BCE(d_f, 0) (today's kernels);  logit D (Discriminator(final_act='none')):
    #               the same objective as F.binary_cross_entropy_with_logits -- no saturating division by p (1 - p)
    #   'lsgan'     mean (d_f - 1)^2 | mean (d_r - r)^2, mean d_f^2; either head (on a sigmoid D the gradient goes back through it)
    #   'hinge'     -mean d_f | mean max(0, 1 - d_r), mean max(0, 1 + d_f); logit D only, r = 1 only (what spectral normalisation
    #               was published with)
    # Everything but vanilla on a sigmoid D is ONE launch per group of terms (engine.gan_loss -> pg_gan_loss: the generator step's term,
    # then the discriminator step's two terms together) in place of two launches per term.  Checked at the top of batch(): ValueError.
    gan_mode = 'vanilla'
    real_label = 1.0

    # Segmentation objectives beyond the reference's three (opt-in): loss_type = 'tversky' | 'weighted_bce' | 'MAE' = off -- the same
    # launches with the same arguments, the same kind key, the same bits, whatever the three settings below hold.  loss_type = 'ce' |
    # 'focal' | 'dice', or a '+'-joined sum of them ('ce+dice', 'focal+dice', ...; each once, none of the reference's three): with p the
    # generator's output, y the target, lp = max(log p, -100), lq = max(log(1 - p), -100), means over the GLOBAL batch B,
    #   'ce'     seg_alpha / (B HW) sum -y lp: categorical cross-entropy on the softmax output (final_act='softmax', >= 2 channels).  A
    #            pixel whose y is all zero has no listed label: it adds nothing and still counts in the normaliser.
    #   'focal'  seg_alpha / (B C HW) sum -(a1 y (1-p)^g lp + a0 (1-y) p^g lq), g = focal_gamma an INTEGER in 0..8 (powers by repeated
    #            multiplication), a1 = focal_alpha, a0 = 1 - focal_alpha, or a1 = a0 = 1 for focal_alpha = None; g = 0 without alpha is
    #            F.binary_cross_entropy.  Sigmoid or softmax head.
    #   'dice'   seg_alpha / (B C) sum_{n,c} (1 - (2 I + s) / (P + Y + s)), I = sum p y, P = sum p, Y = sum y over the pixels of sample n
    #            and channel c, s = dice_smooth > 0: per sample, not per batch.  Sigmoid or softmax head.
    # A sum's value and gradient are the sums of its members' under the one seg_alpha.  Two launches in place of the reference pair
    # (engine.seg_loss_begin / seg_loss_finish -> pg_seg_loss_reduce, pg_seg_loss_value_grad), nothing exchanged under data
    # parallelism, and a window of `accumulate` micro-batches IS the large batch (the objectives are means over samples).  batch() keeps
    # its six keys: the members of a sum are not reported separately.  Checked at the top of batch(): ValueError.
    focal_gamma = 2
    focal_alpha = None
    dice_smooth = 1.0

    # Per-class weights of 'ce' | 'focal' | 'dice' and their sums (opt-in): None = off -- the same launches with the same arguments, the
    # same kind key, the same bits.  A sequence of C numbers w_c (C the generator's output channels; each finite and >= 0 as an fp32
    # number, at least one > 0): every (sample, channel) term of every member is multiplied by w_c,
    #   'ce'     seg_alpha / (B HW) sum_c w_c sum -y_c lp_c    'focal'  seg_alpha / (B C HW) sum_c w_c sum e_c
    #   'dice'   seg_alpha / (B C) sum_{n,c} w_c (1 - D[n,c])
    # in training steps and in evaluate().  The denominators do NOT change with the weights: 'ce' is F.cross_entropy(logits, labels,
    # weight=w, reduction='sum') / (B HW), not torch's reduction='mean', which divides by the sum of the weights of the batch's labelled
    # pixels -- a batch-dependent denominator would need a collective under data parallelism, and a window of `accumulate`
    # micro-batches would stop being the large batch.  The weights enter in the second launch only (pg_seg_loss_value_grad_w in place of
    # pg_seg_loss_value_grad; the reduction pass is unchanged) and live in a device buffer made when the setting is first checked: no
    # copy inside a step.  Changed weights are another kind of step, as a changed focal_gamma is.
    # 'balanced' | 'balanced_sqrt': weights still to be estimated from the data -- estimate_class_weights(data) counts the targets'
    # pixels per class on the device (pg_seg_label_count) and sets w_c proportional to 1 / f_c (1 / sqrt(f_c)), f_c the class's share of
    # the labelled pixels, with mean 1 (engine.class_weights_from_counts); train() does so on its training data before the first epoch,
    # at most class_weight_batches batches of it (None = all), and class_weights.json in the save folder keeps the result for a
    # resumed run (load_last_checkpoint()).
    # With one of the reference's three loss types anything but None is a ValueError (not silently inert), as is a wrong length, a bad
    # value or a scheme name that has not been resolved: checked at the top of batch() / evaluate().
    class_weights = None
    class_weight_batches = None

    # The optimizer's settings (opt-in, beyond the reference, whose optimizers are optim.Adam(lr, betas=(0.9, 0.999))): None = off -- the
    # same launches with the same arguments, the same kind key, the same files.
    #   betas         (beta1, beta2) for both networks, or ((gen_beta1, gen_beta2), (disc_beta1, disc_beta2)); each in [0, 1).  They are
    #                 launch arguments of whichever Adam entry point the step takes (pix2pix: beta1 = 0.5; hinge + spectral
    #                 normalisation: (0.0, 0.9)).
    #   weight_decay  a finite number >= 0 for both networks, or a pair (gen, disc) whose members may be None; 0 / None = that network
    #                 keeps today's entry points.  torch.optim.AdamW(net.parameters(), weight_decay=wd): p *= 1 - lr * wd ahead of the
    #                 moment updates, inside the fused Adam pass (pg_adamw_step: one multiply, no memory access), over the network's WHOLE
    #                 flat parameter buffer -- biases and norm parameters included, with spectral normalisation the stored weight_orig.
    #                 No parameter groups.  The multiplier is formed from the step's own gen_lr / dsc_lr, so lr_decay and the plateau
    #                 schedule carry over; lr * weight_decay must be < 1.
    #   save_optimizer  truthy: save() also writes optimizer_ep_%03d.pth (optimizer_state()) and load_last_checkpoint() reads it back
    #                 (load_optimizer_state()): the next setup_optimizers() -- train() calls it -- then keeps moments and step counts
    #                 instead of zeroing them, and the run resumes exactly.  Off: the files and the behaviour of before, even where
    #                 such a file exists.
    # Checked at the top of batch() and in setup_optimizers(): ValueError.
    betas = None
    weight_decay = None
    save_optimizer = None

    # Gradient accumulation (opt-in, beyond the reference, whose users sum .grad over a few backward() calls before optimizer.step()):
    # None or 1 = off -- no buffer, the same launches, the same kind key, the same bits.  An int k >= 2: every batch(x, y, train=True) is
    # one MICRO-step of a window of k.  It runs the step as ever up to the point where a network's Adam update would launch and returns
    # its own micro-batch's losses; there pg_grad_accum takes the network's flat gradient instead (_adam_step): calls 1 .. k-1 add it
    # into a per-network accumulator (acc = g, then acc += g) and leave weights, moments, the weight average and the step counts alone;
    # call k closes the window -- grad_flat = (acc + g) * fl(1 / k), the window's MEAN gradient -- and everything that sits in front of
    # Adam runs once on that: the norm and skip of clip_grad_norm, AdamW's decay, the update, the weight average; _t_g / _t_d advance
    # by one.  Under data parallelism each call's gradients are all-reduced as today and the REDUCED gradient is accumulated; a
    # spectrally normalised discriminator's gradient is mapped back to the stored weights call by call (each call normalised with its
    # own sigma) before it is added.  By construction: dropout seeds and diffaug draws advance per call; BatchNorm statistics are per
    # micro-batch, as in torch; learning rate, betas and decay are those of the closing call; a NaN in any micro-batch reaches the
    # closed gradient, so with clip_grad_norm set the whole window's update is skipped; where the loss is a mean over the batch (MAE,
    # one-channel weighted BCE, every adversarial term) the window IS the large batch, while loss_type = 'tversky' gives the mean over
    # the window of each micro-batch's own focal-Tversky loss (the power is applied per micro-batch: what accumulating with the
    # reference's loss gives).  Evaluation steps do not touch the window.  step_accumulated() closes a window that is still open
    # (train() does at the end of every epoch's training pass: checkpoints never straddle a window); setup_optimizers(), load(),
    # load_last_checkpoint(), a change of `accumulate` and a training step that raised discard it.  Each phase of the window ('begin',
    # 'add', 'close') is a kind of step of its own: its own launch decision, its own captured graph -- only the closing one holds Adam.
    # Checked at the top of batch(): ValueError.
    accumulate = None

    # Segmentation metrics of evaluation passes (opt-in, beyond the reference): None = off -- no launch, no buffer, no key, file or
    # printed line.  True: every batch(train=False) adds ONE launch beside its segmentation loss (engine.seg_confusion: the confusion
    # counts of G(x) against y, integers, accumulated in `seg_counts` on the device; reset_metrics() / read_metrics()), train() records
    # IoU / Dice / precision / recall / pixel accuracy of every validation pass in `val_history` -- with ema_decay also of the
    # averaged generator (evaluate()) -- and save_best = 'miou' | 'mdice' keeps the best epoch's weights as best_generator.pth /
    # best_discriminator.pth (/ best_generator_ema.pth) with best_metrics.json.  Training steps never launch it.
    metrics = None
    metric_threshold = 0.5   # one-channel masks: prediction >= this is foreground (several channels: the first maximum, no threshold)
    save_best = None
    # Score CURVES of evaluation passes (opt-in; needs metrics = True): None = off -- no launch, no buffer, no key, no printed line.  A
    # power of two in 16..1024: every batch(train=False) adds ONE more launch after its seg_confusion, on the same views
    # (engine.seg_hist: per channel and label a histogram of the prediction over `metric_bins` bins, integers, accumulated in `seg_hist`).
    # read_metrics() / evaluate() then also return metrics.curve() of the table -- IoU / Dice / precision / recall at every threshold
    # k / metric_bins (exactly the counts seg_confusion gives at that threshold), average precision per class, the threshold with the
    # best IoU -- and the table itself; train() prints mean AP and the best threshold, and best_metrics.json carries best_threshold
    # (patchgan_infer's `threshold: best`).  save_best still compares epochs at metric_threshold.
    metric_bins = None

    neptune_config = None
    label_values = None      # label list of the dataset, only for the uint8 (device-side) input path of batch()
    gc_freeze = False        # opt-in: gc.collect() + gc.freeze() after training steps 1 and 3 (_settle_gc; process-global)
    # How a step is launched (decided per KIND of step: shapes, loss settings, precision / tuning, train / eval):
    #   graph        False | True | 'auto'  -- replay the steady-state TRAINING step from a captured hipGraph (_replay): 220 launches become
    #                one hipGraphLaunch (host 1.9 -> 0.1 ms per step).  Only single-GPU steps without dropout can be captured.
    #   two_streams  None | False | True | 'auto'  -- launch by launch with each backward pass's weight-gradient chain (fp32 networks) and
    #                the discriminator step's forward pass on a second stream (engine.Exec).  Independent of capture: dropout, evaluation
    #                passes and data-parallel steps take it too.  None = follows `graph` ('auto' with graph = 'auto', else off).
    # 'auto': a tournament per kind of step.  After one untimed warm step every way of launching that the settings allow -- one stream,
    # two streams, the captured graph -- runs for 2 x TRIAL_STEPS steps (the first half settles: allocator growth for the new pattern) while an event is recorded at the start of each step; a candidate's
    # score is the SHORTEST start-to-start period it reached (the step time as the caller sees it: host-bound or device-bound, whatever
    # binds; the minimum is robust against a loader hiccup or a GC pause in one of the steps), and the fastest candidate is kept.  All
    # candidates are the same computation, bit for bit, so the trials are ordinary training steps.  Measured at cfg2 / cfg4 two streams
    # win (8.3 vs 8.9 ms), at cfg1 too (2.49 ms against 2.92 for the graph: its 219 short kernels leave gaps a second chain fills), a
    # tiny network ends on the graph.  AUTO_FORCE (tests, experiments) decrees the outcome instead of measuring it.
    graph = False
    two_streams = None
    GRAPH_WARM_STEPS = 3     # graph = True: eager steps of a given kind before it is captured (kernel plans, weight-cache plans, workspaces settle)
    TRIAL_STEPS = 4          # 'auto': per candidate, this many settling steps and then this many timed ones
    GRAPH_TRIAL_RATIO = 1.25 # 'auto': the captured graph enters the tournament only if the one-stream step takes < this x its own host enqueue time
    AUTO_FORCE = None        # 'eager1' | 'eager2' | 'graph': 'auto' takes this outcome (where the settings allow it) after the warm steps
    #                          ('graph2' = the two-stream fork / join schedule INSIDE the captured step: by decree only, it is not a tournament
    #                          candidate -- the replay runs its branches no faster than the one-stream capture and slower than the eager
    #                          two-stream step: cfg1 2.96 vs 2.89 vs 2.40 ms, cfg2 8.33 vs 7.02; EXPERIMENTS.md round 6)
    MAX_GRAPHS = 2           # captured kinds of step kept (each holds its activations: ~4 GB at cfg2)
    MAX_KINDS = 16           # kinds of step whose launch decision is remembered
    _hwq_warned = False      # (process-wide: the late GPU_MAX_HW_QUEUES warning is given once)

    def __init__(self, generator, discriminator, savefolder, device='cuda'):
        # (networks that an earlier Trainer drove may still have a discriminator update in flight: complete it before anything here
        #  touches their weights -- the modules' apply() does that through the access hook)
        generator.apply(weights_init)
        discriminator.apply(weights_init)
        self.generator = generator
        self.discriminator = discriminator
        # (a discriminator update may be in flight on the second stream / in a collective when batch() returns: anything that reads the
        #  module's weights through its own surface completes it first.  Hooks chain: an earlier trainer's stays in front of this one's)
        import weakref
        me = weakref.ref(self)
        earlier = getattr(discriminator, '_access_hook', None)

        def hook():
            if earlier is not None:
                earlier()
            t = me()
            if t is not None:
                t.flush()
        discriminator._access_hook = hook
        self.device = device
        if savefolder[-1] != '/':
            savefolder += '/'
        self.savefolder = savefolder
        if not os.path.exists(savefolder):
            os.makedirs(savefolder, exist_ok=True)
        self.start = 1
        self.gen_lr = self.dsc_lr = 1e-3
        self._adam = None          # (gm, gv, dm, dv) flat moment buffers
        self._t_g = self._t_d = 0  # Adam step counts
        self._step = 0
        self._pending_d = None
        self._deferred = None      # operands of a discriminator backward pass still running on the second stream (flush())
        self.bucket_bytes = 32 << 20   # all-reduce bucket size under data parallelism (parallel.GradReducer)
        self._graphs, self._adam_dev = {}, None
        self._kinds, self.step_times, self.launch_mode = {}, None, None      # per kind of step: warm-step count, the tournament, the decision; step_times = the last tournament's ms per step per candidate
        self._exec = None          # engine.Exec: this trainer's workspaces and second stream (created on the networks' device)
        self._oom_kinds, self.oom_fallbacks = set(), 0      # kinds of step pinned to one stream after an out-of-memory two-stream step
        self._ema = self._ema_net = None      # the generator's weight average: flat fp32 buffer + the UNet that views it (ema_decay)
        self.seg_counts = None     # metrics.SegCounts of the evaluation steps since reset_metrics() (created by the first one; `metrics`)
        self.seg_hist = None       # metrics.SegHist of the same evaluation steps (created by the first one; `metric_bins`)
        self.val_history = []      # train() with metrics: one dict per epoch (losses + scores of the validation pass)
        self._best = None          # metrics.BestTracker (save_best)
        self._clip = None          # clip_grad_norm: (status blocks of G and D: 2 x 64 bytes, G's reduction workspace, D's) on the device
        self.grad_history = []     # train() with clip_grad_norm: one read_grad_stats() dict per epoch
        self._aug_counter = None   # diffaug: the step count of the parameter stream, one int64 word on the device (persistent)
        self._aug_params = None    # diffaug: the last training step's parameter table (int32 [N, 8] on the device)
        self._acc = None           # accumulate: the two accumulators (G's, D's), flat fp32 buffers like the gradients
        self._acc_k = None         # ... the window length the open window was begun with
        self._acc_done = 0         # ... training calls completed in the open window (0: none open); host state
        self._acc_cur = None       # ... (phase, gradients in the window with this one) of the training call being enqueued
        self._pending_d_acc = None # ... the place in its window of the call whose D gradient is still in a collective (_pending_d)
        self._acc_run = None       # ... (the configuration, the first step, the last step) of the unbroken run of its training calls
        self._acc_launches = 0     # ... pg_grad_accum launches enqueued so far (the out-of-memory retry of batch() looks at it)
        self._acc_calls = self._acc_updates = 0      # ... training calls / closed windows (what train() prints per epoch)
        self._resume = None        # load_optimizer_state(): moments, step counts and trainer state the next setup_optimizers() takes over
        self._plateau = None       # train(reduce_on_plateau=True): the two _Plateau objects (optimizer_state() records them)
        self._resume_plateau = None      # their restored state, from setup_optimizers() to the train() that called it
        self.class_weight_info = None    # estimate_class_weights(): {'scheme', 'counts', 'unlabelled', 'pixels', 'weights'} of the last estimate

    # -------------------------------------------------------------------------------------- optimizers
    def setup_optimizers(self, gen_lr=1e-3, dsc_lr=1e-3):
        """Fresh Adam state (the reference re-creates both optimizers on every train() call, trainer.py:169-172) -- unless
        load_optimizer_state() left a restored one pending: this call then takes over its moments, step counts, dropout step number and
        augmentation count (the learning rates are this call's arguments) and the state is consumed."""
        self._optim_now((gen_lr, dsc_lr))      # (ValueError before anything changes)
        self.flush()              # an Adam(D) still running on the second stream reads and writes the OLD moments
        self._acc_done = 0        # (accumulate: an open window is discarded -- its gradients belong to the old optimizer state)
        self.gen_lr, self.dsc_lr = gen_lr, dsc_lr
        g, d = self.generator.flat, self.discriminator.flat
        resume, self._resume, self._resume_plateau = self._resume, None, None
        if resume is None:
            self._adam = (torch.zeros_like(g), torch.zeros_like(g), torch.zeros_like(d), torch.zeros_like(d))
            self._t_g = self._t_d = 0
        else:
            self._adam = tuple(t.to(net.device) for t, net in zip(resume['adam'], (g, g, d, d)))
            self._t_g, self._t_d = resume['t_g'], resume['t_d']
            tr = resume['trainer']
            if tr is not None:
                self._step = int(tr['step'])
                if tr.get('diffaug_counter') is not None:
                    self._aug_counter = torch.tensor([int(tr['diffaug_counter'])], dtype=torch.int64, device=g.device)
                self._resume_plateau = tr.get('plateau')
        self._graphs, self._kinds = {}, {}        # captured steps update the OLD moment buffers
        self._ema_ensure()
        if self._clip_ensure():
            self._clip[0].zero_()

    # -------------------------------------------------------------------------------------- betas, weight decay
    _OPTIM_OFF = (((0.9, 0.999), (0.9, 0.999)), (None, None))

    def _optim_now(self, lrs=None):
        """(((gen_beta1, gen_beta2), (disc_beta1, disc_beta2)), (gen_weight_decay, disc_weight_decay)) of the next Adam launches,
        validated (ValueError), the decays also against the learning rates `lrs` (default: the current ones)."""
        if self.betas is None and self.weight_decay is None:
            return self._OPTIM_OFF
        betas, wd = E.check_betas(self.betas), E.check_weight_decay(self.weight_decay)
        for lr, w in zip(lrs if lrs is not None else (self.gen_lr, self.dsc_lr), wd):
            if w is not None:
                E.decay_mul(lr, w)
        return betas, wd

    def _optim_key(self):
        # (betas and the decay are launch arguments of the Adam kernels: a captured step holds the betas it was captured with and,
        #  per network, the entry point with or without a decay.  Off: the key is the one without the feature)
        if self.betas is None and self.weight_decay is None:
            return ()
        return (('optim',) + self._optim_now(),)

    def _opt(self, which):
        """Everything per-network of the optimizer for network `which` ('g' | 'd'), as it stands now: the one place that tells the two
        apart.  Settings are validated (ValueError); m, v, acc and scal are None where the trainer has none (no optimizer yet,
        accumulation off, no step being captured); ema / ema_decay are the generator's alone and None while the average is off."""
        i = 0 if which == 'g' else 1
        decay = self._ema_now() if i == 0 else None
        max_norm = self._clip_now()[i]
        betas, wd = self._optim_now()
        m, v = self._adam[2 * i:2 * i + 2] if self._adam is not None else (None, None)
        scal = self._adam_dev
        if scal is not None:
            k = scal.numel() // 2         # floats per network: 2, or 3 with a decay set (_capture)
            scal = scal[i * k:(i + 1) * k]
        return _Opt(i, (self.generator, self.discriminator)[i], m, v, (self._t_g, self._t_d)[i], (self.gen_lr, self.dsc_lr)[i], betas[i], wd[i],
                    max_norm, self._ema if decay is not None else None, decay, self._acc[i] if self._acc is not None else None, scal)

    def _opt_buffers(self):
        """The optimizer's device buffers in use now: the moments, the weight average while it is on, clipping's status blocks and
        workspaces while either network clips (else three Nones: the places stay), the accumulators inside a window.  What a captured
        step keeps alive besides the gradients, and by whose addresses it is recognised as stale."""
        ema = self._ema if self._ema_now() is not None else None
        clip = tuple(self._clip) if (self._clip is not None and self._clip_now() != (None, None)) else (None, None, None)
        acc = tuple(self._acc) if (self._acc is not None and self._acc_cur is not None) else ()
        return tuple(self._adam) + clip + (ema,) + acc

    def _adam_scalars(self, which, k):
        """The `k` floats (2, or 3 with a decay set for either network) a captured step's Adam launch of network `which` reads."""
        o = self._opt(which)
        sc = E.adam_scalars(o.t, o.lr, o.betas[0], o.betas[1], o.weight_decay)
        return sc + (np.float32(1.0),) * (k - len(sc))

    # -------------------------------------------------------------------------------------- gradient-norm clipping
    def _clip_now(self):
        """(gen_max_norm, disc_max_norm) of the next Adam launches, each None (the plain launch) or the validated float."""
        if self.clip_grad_norm is None:
            return None, None
        return E.check_clip_norm(self.clip_grad_norm)

    def _clip_ensure(self):
        """With clip_grad_norm set: the persistent device buffers (created zeroed, re-created on another device).  -> whether they exist."""
        if self._clip_now() == (None, None):
            return self._clip is not None
        G, D = self.generator, self.discriminator
        dev = G.flat.device
        if self._clip is None or self._clip[0].device != dev:
            self.flush()
            ws = [torch.zeros(max(E.grad_norm_workspace_bytes(net.flat.numel()) // 8, 1), dtype=torch.float64, device=dev) for net in (G, D)]
            # (one workspace per network: in a two-stream step Adam(G) and Adam(D) run on different streams at the same time)
            self._clip = (torch.zeros(2 * E.GRAD_STAT.itemsize // 8, dtype=torch.float64, device=dev), ws[0], ws[1])
        return True

    def _clip_stat(self, which):
        k = E.GRAD_STAT.itemsize // 8
        return self._clip[0][0:k] if which == 'g' else self._clip[0][k:2 * k]

    def read_grad_stats(self):
        """{'gen': {...}, 'disc': {...}}: norm and coef of the last step, and since reset_grad_stats() / setup_optimizers() the counts
        `steps`, `clipped` (coef < 1), `skipped` (non-finite gradient: nothing was written), `max_norm` and `mean_norm` over the steps
        with a finite norm.  Completes a discriminator update in flight, copies 128 bytes and waits for the device."""
        if self._clip_now() == (None, None) or not self._clip_ensure():
            raise RuntimeError("read_grad_stats(): Trainer.clip_grad_norm is None (gradient-norm clipping is off)")
        self.flush()
        rec = self._clip[0].cpu().numpy().view(E.GRAD_STAT)
        out = {}
        for name, r in zip(('gen', 'disc'), rec):
            finite = int(r['steps']) - int(r['skipped'])
            out[name] = dict(norm=float(r['norm']), coef=float(r['coef']), steps=int(r['steps']), clipped=int(r['clipped']),
                             skipped=int(r['skipped']), max_norm=float(r['max_norm']),
                             mean_norm=float(r['sum_norm']) / finite if finite else float('nan'))
        return out

    def reset_grad_stats(self):
        """Clear the accumulators of read_grad_stats()."""
        if self._clip_now() == (None, None) or not self._clip_ensure():
            raise RuntimeError("reset_grad_stats(): Trainer.clip_grad_norm is None (gradient-norm clipping is off)")
        self.flush()
        self._clip[0].zero_()

    # -------------------------------------------------------------------------------------- gradient accumulation
    def _acc_now(self):
        """The window length of the next training call: None (off: `accumulate` None or 1) or the validated int >= 2."""
        if self.accumulate is None:
            return None
        return E.check_accumulate(self.accumulate)

    def _acc_ensure(self):
        """With accumulate set: one accumulator per network (created zeroed outside any capture, re-created when a network moved or
        changed its size).  -> whether they exist."""
        if self._acc_now() is None:
            return self._acc is not None
        flats = (self.generator.flat, self.discriminator.flat)
        if self._acc is None or any(a.device != f.device or a.numel() != f.numel() for a, f in zip(self._acc, flats)):
            self.flush()
            self._acc = tuple(torch.zeros_like(f) for f in flats)
            self._acc_done = 0    # (whatever an open window held went with the old buffers)
        return True

    def _acc_begin_call(self):
        """At the top of a training call: (phase, gradients in the window once this call's is in) or None with accumulation off.  A
        window begun with another length is discarded: this call begins a new one."""
        k = self._acc_now()
        if k != self._acc_k:
            self._acc_k, self._acc_done = k, 0
        if k is None:
            return None
        self._acc_ensure()        # (never allocated inside a capture)
        return E.accum_phase(self._acc_done, k), self._acc_done + 1

    def _acc_key(self):
        # (the phase decides which launches the step holds -- the non-closing ones have no Adam --, k is the closing launch's scale:
        #  every phase is a kind of step of its own.  Off: the key is the one without the feature)
        cur = self._acc_cur
        return (('accum', self._acc_k, cur[0]),) if cur is not None else ()

    def step_accumulated(self):
        """Close a window that is still open after c < k training calls: grad_flat = acc * fl(1 / c) for both networks (pg_grad_accum's
        PG_ACC_CLOSE_ONLY), then what the closing call of a full window does -- clipping's norm and skip, the decay, Adam, the weight
        average, one step count.  Launch by launch on the current stream, after flush().  -> whether there was a window to close."""
        self.flush()
        c = self._acc_done
        if c == 0 or self._acc_now() is None or self._acc is None:
            self._acc_done = 0
            return False
        self._acc_done = 0
        for which in ('g', 'd'):
            self._adam_step(which, acc=('close_only', c))
        self._acc_updates += 1
        return True

    # -------------------------------------------------------------------------------------- differentiable augmentation
    def _aug_now(self):
        """None (off) or (policy bits, seed) of the next training step, both validated."""
        if self.diffaug is None:
            return None
        bits = E.diffaug_policy(self.diffaug)
        return (bits, E.diffaug_seed(self.diffaug_seed)) if bits else None

    def _aug_ensure(self):
        """With diffaug set: the persistent step-count word (created zeroed outside any capture, re-created on another device)."""
        if self._aug_now() is None:
            return
        dev = self.generator.flat.device
        if self._aug_counter is None or self._aug_counter.device != dev:
            self._aug_counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def _aug_begin(self, aug, din, real, rank):
        """The step's parameter table and the augmented discriminator input, on the current stream: one parameter launch, din_aug
        allocated beside din (same shape and pixel stride: its halves keep din's 16-byte phase relation) and its real half filled.
        -> (din_aug, its real half, its fake half -- still to be filled once the generator has written din's --, the table)."""
        N = real.N
        self._aug_ensure()
        params = self._aug_params = E.diffaug_params(aug[1], self._aug_counter, 0, aug[0], rank * N, N, real.H, real.W)
        # (8-float pixels of fewer channels: the pad channels are zero as din's are)
        t = (torch.zeros if din.ld != din.C else torch.empty)(din.N * din.H * din.W * din.ld, dtype=torch.float32, device=din.t.device)
        din_aug = E.View(t, 0, din.ld, din.N, din.H, din.W, din.C)
        real_aug, fake_aug = din_aug.samples(0, N), din_aug.samples(N, N)
        E.diffaug_fwd(real, real_aug, params, 0)
        return din_aug, real_aug, fake_aug, params

    def read_diffaug_params(self):
        """The parameter table of the last training step: int32 NumPy array [N, 8], rows {flip, ty, tx, cut_top, cut_left, cut_h, cut_w,
        0} of this rank's samples (one synchronising copy; for tests and inspection)."""
        if self._aug_params is None:
            raise RuntimeError("read_diffaug_params(): no training step with Trainer.diffaug set has run")
        return self._aug_params.cpu().numpy().copy()

    # -------------------------------------------------------------------------------------- the adversarial objective
    def _gan_now(self):
        """(gan_mode, real_label, the discriminator's final_act) of the next step, validated (ValueError)."""
        fa = self.discriminator.final_act
        return E.check_gan_mode(self.gan_mode, self.real_label, fa) + (fa,)

    # -------------------------------------------------------------------------------------- the segmentation objective
    def _seg_now(self):
        """None while loss_type is one of the reference's three, else the validated engine.SegLossSpec of the next step (ValueError)."""
        ge = self.generator.engine
        if self.class_weights is None:
            return E.check_seg_loss(self.loss_type, ge.final_act, ge.output_nc, self.focal_gamma, self.focal_alpha, self.dice_smooth)
        # (the weights' device buffer is made here, by the check at the top of batch() / evaluate(): later checks of the step find it)
        return E.check_seg_loss(self.loss_type, ge.final_act, ge.output_nc, self.focal_gamma, self.focal_alpha, self.dice_smooth,
                                self.class_weights, self.generator.flat.device)

    # -------------------------------------------------------------------------------------- per-class weights from the data
    CLASS_WEIGHTS_FILE = 'class_weights.json'

    def estimate_class_weights(self, data, scheme='balanced', max_batches=None):
        """Per-class weights from the targets of `data` (an iterable of (x, y) batches as batch() takes them): every target is uploaded
        as a step uploads it and counted on the device (one pg_seg_label_count launch per batch into one table; the counts are read
        once, at the end), under a process group every rank counts its shard and the tables are summed by one int64 all-reduce (a
        COLLECTIVE outside any step: every rank calls it).  -> the weights engine.class_weights_from_counts(counts, scheme) gives, also
        set as Trainer.class_weights; `class_weight_info` keeps scheme, counts and weights, and rank 0 writes them to
        class_weights.json in the save folder.  max_batches: count at most that many batches (None = all)."""
        if scheme not in E.CLASS_WEIGHT_SCHEMES:
            raise ValueError(f"scheme must be one of {' | '.join(E.CLASS_WEIGHT_SCHEMES)}, not {scheme!r}")
        if max_batches is not None and (isinstance(max_batches, bool) or not isinstance(max_batches, int) or max_batches < 1):
            raise ValueError(f"max_batches must be None or an integer >= 1, not {max_batches!r}")
        G = self.generator
        C, dev = G.engine.output_nc, G.flat.device
        if C < 2:
            raise ValueError("estimate_class_weights(): one output channel has nothing to be balanced against")
        self.flush()
        dist = _dist()
        counts = torch.zeros(C + 2, dtype=torch.int64, device=dev)
        for i, (x, y) in enumerate(data):
            if max_batches is not None and i >= max_batches:
                break
            x, y, u8, N, H, W, Cin, Cout = self._inputs(x, y)
            yv = E.View.alloc(N, H, W, Cout, dev)
            if u8:
                yv.from_labels(y, self.label_values)
            else:
                yv.from_nchw(y)
            E.seg_label_count(yv, counts)
        if dist.on:
            if dist.backend != 'nccl':
                counts = counts.cpu()
            dist.dist.all_reduce(counts, op=dist.dist.ReduceOp.SUM)
        a = [int(v) for v in counts.cpu().numpy()]
        weights = E.class_weights_from_counts(a[:C], scheme)
        self.class_weight_info = {'scheme': scheme, 'counts': a[:C], 'unlabelled': a[C], 'pixels': a[C + 1], 'weights': weights}
        self.class_weights = list(weights)
        if dist.rank == 0:
            import json
            with open(self.savefolder + self.CLASS_WEIGHTS_FILE, 'w') as f:
                json.dump(self.class_weight_info, f, indent=1)
        return list(weights)

    def _class_weights_restore(self):
        """class_weights.json of the save folder, where the setting is the scheme name it was estimated with: the weights of the earlier
        run (a resumed run does not re-draw the estimate from randomly cropped data).  -> whether they were taken."""
        path = self.savefolder + self.CLASS_WEIGHTS_FILE
        if not isinstance(self.class_weights, str) or not os.path.exists(path):
            return False
        import json
        with open(path) as f:
            info = json.load(f)
        C = self.generator.engine.output_nc
        if info.get('scheme') != self.class_weights or len(info.get('weights', ())) != C:
            return False
        self.class_weights = list(E.check_class_weights(info['weights'], C))
        self.class_weight_info = info
        print(f"Loaded the class weights from {self.CLASS_WEIGHTS_FILE}: {self.class_weights}")
        return True

    def _seg_begin(self, spec, gen, yv, allred):
        """Phase 1 of the segmentation loss: the reference pair's, or the new objectives' (spec = _seg_now())."""
        if spec is None:
            return E.loss_begin(gen, yv, 0.0, self.tversky_beta, allred)
        return E.seg_loss_begin(gen, yv, spec)

    def _seg_finish(self, spec, pending, grad_out, loss_out, bglobal):
        """Phase 2: the value into loss_out[0] and, with grad_out, the gradient wrt the generator's output."""
        if spec is None:
            return E.loss_finish(pending, _LOSS_MODES[self.loss_type], float(self.seg_alpha), grad_out, loss_out, 0, bglobal,
                                 self.tversky_gamma)
        return E.seg_loss_finish(pending, float(self.seg_alpha), grad_out, loss_out, 0, bglobal)

    # -------------------------------------------------------------------------------------- the generator's weight average
    @property
    def ema_generator(self):
        """UNet (eval mode) on the averaged weights; None while ema_decay is None or before the state exists.  Its parameters are
        views of the buffer G's Adam kernel updates in place, so state_dict() / forward() / predict_image() see the current average.
        No access hook is needed: Adam(G) is enqueued on the main stream in every launch mode (one stream, two streams -- also when
        it moves behind the fork of the deferred discriminator pass --, a replayed capture, data parallelism), so whatever reads the
        average on the current stream is ordered behind the update.  A BatchNorm generator's running statistics are the live
        generator's own tensors."""
        return self._ema_net if self.ema_decay is not None else None

    def _ema_now(self):
        """The decay G's next Adam launch carries: None (plain pg_adam_step) or the validated float."""
        if self.ema_decay is None:
            return None
        decay = E.check_ema_decay(self.ema_decay)
        return decay if self._ema is not None else None      # (set after setup_optimizers(): it starts with the next one)

    def _ema_ensure(self):
        """Create the average (a copy of the live weights) if ema_decay asks for one and none exists; keep an existing one on the
        generator's device, precision, tuning and BatchNorm buffers.  Draws nothing from torch's RNG."""
        if self.ema_decay is None:
            return
        E.check_ema_decay(self.ema_decay)
        G = self.generator
        if self._ema is None:
            self.flush()
            self._ema = G.flat.detach().clone()
            self._ema_net = G.twin(self._ema)
        else:
            if self._ema.device != G.flat.device:
                self._ema = self._ema.to(G.flat.device)
            self._ema_net.follow(G, self._ema)

    def reset_ema(self):
        """Restart the average from the live generator weights."""
        if self.ema_decay is None:
            raise RuntimeError("reset_ema(): Trainer.ema_decay is None (the weight average is off)")
        fresh = self._ema is None
        self._ema_ensure()            # (a new average starts as a copy already)
        if not fresh:
            self.flush()
            self._ema.copy_(self.generator.flat)

    # -------------------------------------------------------------------------------------- segmentation metrics
    def _seg_counts(self):
        """The counts evaluation steps add to, created on first use (on the generator's device, for its output channels)."""
        G = self.generator
        sc = self.seg_counts
        if sc is None or sc.C != G.engine.output_nc or sc.t.device != G.flat.device:
            sc = self.seg_counts = SegCounts(G.engine.output_nc, G.flat.device)
        return sc

    def _metric_bins(self):
        """Trainer.metric_bins checked: None (off) or the bin count as an int.  ValueError for anything else, and without `metrics`."""
        if self.metric_bins is None:
            return None
        bins = check_bins(self.metric_bins)
        if bins is None:
            raise ValueError(f"Trainer.metric_bins = {self.metric_bins!r} must be None or a power of two in 16 .. 1024")
        if not self.metrics:
            raise ValueError(f"Trainer.metric_bins = {self.metric_bins!r} needs Trainer.metrics = True (the histograms are built beside the validation counts)")
        return bins

    def _seg_hist(self, bins):
        """The histogram table evaluation steps add to, created on first use (as _seg_counts; a changed bin count starts a new one)."""
        G = self.generator
        sh = self.seg_hist
        if sh is None or sh.C != G.engine.output_nc or sh.bins != bins or sh.t.device != G.flat.device:
            sh = self.seg_hist = SegHist(G.engine.output_nc, bins, G.flat.device)
        return sh

    def reset_metrics(self):
        """Zero the counts of the evaluation steps (Trainer.metrics) and, with metric_bins, their histograms; the validation pass of
        train() starts with it."""
        self._seg_counts().zero_()
        bins = self._metric_bins()
        if bins is not None:
            self._seg_hist(bins).zero_()

    def read_metrics(self):
        """Scores of the evaluation steps since reset_metrics(): metrics.scores() of their confusion matrix plus `confusion` (np.int64
        [K, K], [true class][predicted class]) and `ignored`; with metric_bins also the keys of metrics.curve() and `hist` (np.int64
        [C, 2, bins]).  Waits for the device; under data parallelism the ranks' counts are summed, which is a collective: every rank
        calls it."""
        out = report(*self._seg_counts().read(_dist()))
        bins = self._metric_bins()
        if bins is not None:
            out.update(report_curve(self._seg_hist(bins).read(_dist())[0]))
        return out

    def evaluate(self, data, generator=None):
        """A generator-only pass over `data` (an iterable of (x, y) batches as batch() takes them): no discriminator, no update.
        `generator`: any UNet of the live generator's geometry on its device -- None = the live one, `trainer.ema_generator` the
        intended other.  It runs in eval mode (restored afterwards).  Per batch: one generator forward writing into the view an
        evaluation batch() uses (so its head layer runs the same kernel: the pass is bit-comparable to batch(train=False)), the
        segmentation loss by batch()'s own calls, and the confusion counts -- into counts of this call's own, not `seg_counts`.
        With metric_bins the histograms as well, into a table of this call's own.
        Nothing is read back per batch: the loss values are summed on the device.  Returns {'seg_loss': mean over the batches,
        **scores, 'confusion', 'ignored'} (with metric_bins: + the keys of metrics.curve() and 'hist'); under data parallelism every rank passes its shard and gets the global result (collective)."""
        net = self.generator if generator is None else generator
        G = self.generator
        ge, dev = net.engine, G.flat.device
        if (ge.input_nc, ge.output_nc) != (G.engine.input_nc, G.engine.output_nc) or net.flat.device != dev:
            raise RuntimeError("evaluate(): the generator must have the live generator's channels and device")
        seg_spec = self._seg_now()      # (ValueError before anything is launched)
        self.flush()
        dist = _dist()
        counts = SegCounts(ge.output_nc, dev)
        bins = self._metric_bins()
        hist = SegHist(ge.output_nc, bins, dev) if bins is not None else None
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        allred = dist.all_reduce_side if dist.on else None
        ex = self._exec
        if ex is None or ex.device != dev:
            ex = self._exec = E.Exec(dev)
        was_training, nbatches = net.training, 0
        net.eval()
        try:
            with ex:
                for x, y in data:
                    x, y, u8, N, H, W, Cin, Cout = self._inputs(x, y)
                    din, real, fake = self._din(x, y, u8, N, H, W, Cin, Cout)
                    xin, yv, gen = fake.channels(0, Cin), real.channels(Cin, Cout), fake.channels(Cin, Cout)
                    loss = torch.empty(1, dtype=torch.float32, device=dev)
                    ge.forward(net.flat, xin, gen, False, 0, sample0=dist.rank * N, bn=net.bn_run())
                    pending = self._seg_begin(seg_spec, gen, yv, allred)
                    E.seg_confusion(gen, yv, self.metric_threshold, counts.t)
                    if hist is not None:
                        E.seg_hist(gen, yv, bins, hist.t)
                    self._seg_finish(seg_spec, pending, None, loss, N * dist.world)
                    total += loss
                    nbatches += 1
        finally:
            net.train(was_training)
        if dist.on and self.loss_type != 'tversky':
            # (focal-Tversky's value is global on every rank already; the others are per-rank partial means: batch() sums them too)
            if dist.backend != 'nccl':
                total = total.cpu()
            dist.dist.all_reduce(total, op=dist.dist.ReduceOp.SUM)
        out = report(*counts.read(dist))
        if hist is not None:
            out.update(report_curve(hist.read(dist)[0]))
        seg = float(total.cpu()[0]) / nbatches if nbatches else float('nan')
        return dict({'seg_loss': seg}, **out)

    # -------------------------------------------------------------------------------------- one G+D step
    def _inputs(self, x, y):
        """One batch as batch() / evaluate() take it, on the generator's device: (x, y, u8, N, H, W, Cin, Cout)."""
        G, D = self.generator, self.discriminator
        dev = G.flat.device
        if dev.type != 'cuda':
            raise RuntimeError("patchgan_amd.Trainer needs the networks on a HIP device (generator.to('cuda')); "
                               "there is no CPU path")
        if any(e.has_bn and not e.sync_bn for e in (G.engine, D.engine)) and _dist().on:
            # per-rank batch statistics would break "the sum over ranks is the large batch's step" (parallel.py): only the opt-in
            # nn.SyncBatchNorm layer type, which normalises with the global batch's statistics, passes
            raise NotImplementedError("patchgan_amd: data parallelism is not implemented for nn.BatchNorm2d networks "
                                      "(build them with norm_layer=nn.SyncBatchNorm: the same state_dict, global batch statistics)")
        # device-side input pipeline (opt-in, beyond the reference): decoded bytes x uint8 [N,H,W,Cin] + label map y uint8
        # [N,H,W]; `/255.` and the one-hot mask over self.label_values (io.py:42-56) run on the GPU after a 4x smaller H2D
        u8 = isinstance(x, torch.Tensor) and x.dtype == torch.uint8
        if u8:
            if self.label_values is None:
                raise RuntimeError("uint8 input needs Trainer.label_values (the dataset's label list)")
            x = x.to(dev, non_blocking=True)
            y = y.to(dev, non_blocking=True)
            N, H, W, Cin = x.shape
            Cout = len(self.label_values)
        else:
            if not isinstance(x, torch.Tensor):
                x = torch.as_tensor(np.asarray(x), dtype=torch.float)
                y = torch.as_tensor(np.asarray(y), dtype=torch.float)
            x = x.to(dev, dtype=torch.float32, non_blocking=True)
            y = y.to(dev, dtype=torch.float32, non_blocking=True)
            N, Cin, H, W = x.shape
            Cout = y.shape[1]
        ge, de = G.engine, D.engine
        if Cin != ge.input_nc or Cout != ge.output_nc or Cin + Cout != de.input_nc:
            raise RuntimeError(f"channel mismatch: x {Cin}, y {Cout} vs generator ({ge.input_nc}->{ge.output_nc}), "
                               f"discriminator input {de.input_nc}")
        return x, y, u8, N, H, W, Cin, Cout

    def batch(self, x, y, train=False):
        t_host0 = time.perf_counter()
        G, D = self.generator, self.discriminator
        self._gan_now()           # (ValueError before anything is launched)
        self._seg_now()           # (likewise)
        self._optim_now()         # (likewise)
        self._acc_now()           # (likewise)
        if not train and self.metric_bins is not None:
            self._metric_bins()   # (an evaluation step: ValueError before anything is launched)
        x, y, u8, N, H, W, Cin, Cout = self._inputs(x, y)
        dev = G.flat.device
        if train and self._adam is None:
            self.setup_optimizers(self.gen_lr, self.dsc_lr)
        if train and self._ema is not None and self.ema_decay is not None:
            self._ema_ensure()    # (a generator moved / re-tuned since: the average follows)
        if train and self.clip_grad_norm is not None:
            self._clip_ensure()   # (set after setup_optimizers(), or the networks moved: never allocated inside a capture)
        if train and self.diffaug is not None:
            self._aug_ensure()    # (the step-count word: never allocated inside a capture)
        # accumulate: this call's place in its window (None = off); evaluation steps neither read nor move it
        acc = self._acc_cur = self._acc_begin_call() if train else None
        self._step += 1
        ex = self._exec
        if ex is None or ex.device != dev:
            self.flush()          # (a deferred pass is joined on the Exec it was enqueued on, before that one is let go)
            ex = self._exec = E.Exec(dev)
        with ex:
            dims = (N, H, W, Cin, Cout)
            key = self._kind_key(x, y, u8, dims, train)
            if acc is not None:
                # (the run of calls of this configuration -- the key without the phase -- and the step it began with: _launch_mode)
                if self._acc_run is None or self._acc_run[0] != key[:-1] or self._acc_run[2] != self._step - 1:
                    self._acc_run = (key[:-1], self._step, self._step)
                else:
                    self._acc_run = self._acc_run[:2] + (self._step,)
            mode = self._launch_mode(key, train)
            losses = None
            try:
                if mode in ('graph', 'graph2'):
                    losses = self._replay(key, x, y, u8, dims, two=(mode == 'graph2'))   # None: this runtime cannot capture the step
                    if losses is None:
                        mode = 'eager1'
                if losses is None:
                    ex.enabled = mode == 'eager2'
                    t_g0, t_d0, acc0 = self._t_g, self._t_d, self._acc_launches
                    try:
                        losses = self._enqueue_step(x, y, u8, N, H, W, Cin, Cout, train)
                    except torch.cuda.OutOfMemoryError:
                        # the two-stream step holds ~2x the one-stream step's memory (second workspace, the early discriminator forward
                        # beside the generator's saved activations): where it does not fit, this KIND of step runs on one stream from
                        # now on.  Safe to run again only while nothing of this step was committed (no optimizer update enqueued, and
                        # with `accumulate` no gradient added to its window).
                        if mode != 'eager2' or _dist().on or (self._t_g, self._t_d, self._acc_launches) != (t_g0, t_d0, acc0):
                            raise
                        self._two_stream_oom(ex, key)
                        mode = 'eager1'
                        losses = self._enqueue_step(x, y, u8, N, H, W, Cin, Cout, train)
                    finally:
                        ex.enabled = False
            except BaseException:
                kind = self._kinds.get(key)
                if kind is not None:
                    kind['trial'] = None          # a step that raised must not score in a running tournament: it starts over
                if acc is not None:
                    self._acc_done = 0            # ... and what it may have added to an open window is discarded with the window
                raise
            finally:
                self._acc_cur = None
            self.launch_mode = mode
        if acc is not None:
            # the window position advances once per completed training call
            self._acc_done = 0 if acc[0] == 'close' else acc[1]
            self._acc_calls += 1
            self._acc_updates += acc[0] == 'close'
        if train and self.gc_freeze:
            _settle_gc(self._step)
        self.host_ms = (time.perf_counter() - t_host0) * 1e3       # host time to enqueue the whole step (bench.py reports it)
        kind = self._kinds.get(key)
        if kind is not None and kind.get('trial') is not None:
            h = kind['trial']['host']
            h[mode] = min(h.get(mode, 1e30), self.host_ms)
        return self._publish(losses)

    marks = None             # diagnostics (tools/step_phases.py): a list -> every _mark(name) records an event on the current stream

    def _mark(self, name):
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev, time.perf_counter()))

    def _din(self, x, y, u8, N, H, W, Cin, Cout):
        """The discriminator input buffer of one step, filled from the device-resident inputs: (din, real, fake) with samples [0,N)
        real = x|y and [N,2N) fake = x|G(x) (trainer.py:65,96,98), the generator's output channels still to be written."""
        dev = self.generator.flat.device
        de = self.discriminator.engine
        Cd = Cin + Cout
        # (bf16 networks read it through pg_pad8_bf16: 8-float pixels there, so that pass and the fill below move whole 16-byte pieces)
        ld_din = 8 if (4 < Cd < 8 and (de.algo & L.ALGO_MASK) == L.ALGO_BF16) else Cd
        din = E.View(torch.empty(2 * N * H * W * ld_din, dtype=torch.float32, device=dev), 0, ld_din, 2 * N, H, W, Cd)
        real, fake = din.samples(0, N), din.samples(N, N)
        if u8:
            real.channels(0, Cin).from_u8(x)
            fake.channels(0, Cin).from_u8(x)
            real.channels(Cin, Cout).from_labels(y, self.label_values)
        elif Cd <= 8:
            E.din_fill(x, y, real, fake)       # both halves' x | y (and the fake half's zeroed mask channels) in one launch
        else:
            real.channels(0, Cin).from_nchw(x)
            fake.channels(0, Cin).from_nchw(x)
            real.channels(Cin, Cout).from_nchw(y)
        return din, real, fake

    def _enqueue_step(self, x, y, u8, N, H, W, Cin, Cout, train):
        """Every launch of one step on the current stream, from the device-resident inputs to the four loss scalars (returned as a
        device tensor).  Nothing in here reads the device; the only step-dependent HOST values are the dropout seed (self._step) and
        Adam's step count / learning rate (_adam_step) -- with dropout off and self._adam_dev set the sequence is the same from step
        to step, which is what _batch_graph captures."""
        G, D = self.generator, self.discriminator
        ge, de = G.engine, D.engine
        dev = G.flat.device
        dist = _dist()
        if dist.on and not Trainer._hwq_warned:
            Trainer._hwq_warned = True
            import patchgan_amd
            if patchgan_amd.HWQ_LATE:
                import warnings
                warnings.warn('patchgan_amd: HIP was initialised before `import patchgan_amd`, so GPU_MAX_HW_QUEUES=8 could not take effect; '
                              'the data-parallel step keeps five streams busy and loses ~0.6 ms per step at cfg2 with the default 4 hardware '
                              'queues -- import patchgan_amd first or export GPU_MAX_HW_QUEUES=8')
        Bglobal = N * dist.world
        ex = E.cur_exec(dev)
        self._mark('start')

        din, real, fake = self._din(x, y, u8, N, H, W, Cin, Cout)
        xin, yv, gen = fake.channels(0, Cin), real.channels(Cin, Cout), fake.channels(Cin, Cout)
        # differentiable augmentation (training steps with Trainer.diffaug): every D pass below reads din_d = T(din) instead of din.  The
        # table and the real half (x | y only) are made here, on this stream, ahead of the fork of the early D forward; the fake half
        # follows the generator forward; real sample i and fake sample i share row i.  Off: din_d IS din -- no launch, no buffer.
        aug = self._aug_now() if train else None
        if aug is not None:
            din_d, real_d, fake_d, aug_params = self._aug_begin(aug, din, real, dist.rank)
        else:
            din_d, real_d, fake_d, aug_params = din, real, fake, None

        losses = torch.empty(4, dtype=torch.float32, device=dev)   # seg, gdisc, real*0.5, fake*0.5 (each written by its loss kernel)
        # the adversarial objective: kind_g / kind_d None = nn.BCELoss on the sigmoid map (the reference), else the terms of pg_gan_loss
        gan_mode, real_label, d_act = self._gan_now()
        kind_g, kind_d = E.gan_kinds(gan_mode, d_act)
        allred = dist.all_reduce_side if dist.on else None

        # ---- generator step
        seed = E._mix_seed(G._seed_base, self._step) if G.training else 0
        # G's weights are constant from here to its Adam step: its Winograd-transformed / packed bf16 weights for this step are made by
        # one batched launch (from the second step on; engine._WeightPrep), shared by forward and backward where one copy serves both
        gcache = ge.ucache_begin(G.flat, N, H, W) if train else None
        gc = ge.forward(G.flat, xin, gen, G.training, seed, sample0=dist.rank * N, keep_v=train, ucache=gcache,
                        bn=G.bn_run())                                                        # trainer.py:63
        G.bn_update(1)        # BatchNorm generator in training mode: its one running-statistics update of the step
        if aug is not None:
            E.diffaug_fwd(fake, fake_d, aug_params, 0)      # x | G(x) under the rows of the real samples it is paired with
        self._mark('G fwd done')
        self.flush()          # D's deferred all-reduce + Adam from the previous step ran under this G forward
        self._mark('flushed')
        # D's weights as the step's passes read them.  A spectrally normalised discriminator (Discriminator(spectral_norm=True)): ONE
        # normalisation per call, here -- behind the previous step's Adam(D), ahead of the fork of the early D forward --, with one power
        # iteration when D is in training mode; every D pass of this call, forward and backward, and the weight preparation read that
        # one buffer (a stable address).  Otherwise the flat buffer itself: no launch.
        dw = D.spectral_normalize() if de.spectral else D.flat
        # seg loss, phase 1 (per-sample reductions); under data parallelism its two batch-global terms are summed across
        # ranks on the comm stream while the discriminator's forward pass over the fake batch runs
        seg_spec = self._seg_now()
        seg_pending = self._seg_begin(seg_spec, gen, yv, allred)
        if self.metrics and not train:
            # evaluation step: the confusion counts of G(x) against y, one more pass over the bytes the loss reduction just read (on this
            # stream in every launch mode; never in a training step, so a captured step does not hold it)
            E.seg_confusion(gen, yv, self.metric_threshold, self._seg_counts().t)
            bins = self._metric_bins()
            if bins is not None:
                # (the histograms every threshold's counts follow from: one more pass over the same bytes, on this stream as well)
                E.seg_hist(gen, yv, bins, self._seg_hist(bins).t)
        # D's weights do not change until the Adam step at the end of this call: its Winograd-transformed weights are computed
        # once per (layer, direction) and shared by the passes below through this per-step cache
        ucache = de.ucache_begin(dw, N, H, W, tag=bool(train))
        # two-stream step: the discriminator step's forward over din[2N] (trainer.py:96-99) needs only the generator's OUTPUT and D's
        # weights, both final here -- it is enqueued on the second stream now and runs under the rest of the generator step (same
        # kernels, same 2N plan: bit-identical); joined where the discriminator step reads its output
        dc2 = None
        # shared pass: the step's ONE context over din[2N]; its fake half is filled on this stream where the generator step needs it, its
        # real half (x | y and D's weights only) wherever the 2N pass would run.  Its tensors are allocated here, on this stream, before
        # the fork: both streams write into them, and they are released only after the streams have joined.
        # (both halves of din on one 16-byte phase: the first layer then takes the same kernel for either as for the whole buffer)
        shared = (de.context(dw, din_d, keep_v=train)
                  if (SHARE_D_FAKE and de.halves_ok(N, H, W) and (fake_d.ptr() - real_d.ptr()) % 16 == 0) else None)
        real_done = False
        # (evaluation passes and data-parallel steps too; under data parallelism D's deferred update of the previous step has been
        #  applied by flush() above, and on_side() orders the second stream behind it)
        if ex.enabled and E.PROFILER is None and EARLY_D_FWD:      # (bf16 networks too: 5.93 -> 5.84 ms at cfg4)
            n_prepared = len(ucache)
            with E.on_side():
                if shared is not None:
                    de.forward_part(dw, shared, 0, N, ucache=ucache)
                    real_done = True
                else:
                    dc2 = de.forward(dw, din_d, ucache=ucache, keep_v=train, bn=D.bn_run(1, 2))
                self._mark('side: dc2 fwd done')
            if len(ucache) != n_prepared:
                # (a transformed-weight entry the batched preparation did not cover was made by a kernel on the second stream -- the
                #  first steps after a change of tuning: the passes below would take it as ready, so they wait for it this once)
                E.side_join()
        # (BatchNorm discriminator: this pass's batch statistics go to slot 0, the 2N pass's halves to slots 1 and 2 -- the order of the
        #  reference's three calls, trainer.py:66,97,99, whichever pass runs first here)
        if shared is not None:
            de.forward_part(dw, shared, N, N, ucache=ucache)                                  # trainer.py:66 (and the fake half of :98-99)
            dc = shared.samples(N, N)
        else:
            dc = de.forward(dw, fake_d, ucache=ucache, bn=D.bn_run(0, 1))                     # trainer.py:66
        gseg = E.View.alloc(N, H, W, Cout, dev) if train else None
        self._seg_finish(seg_spec, seg_pending, gseg, losses, Bglobal)                        # trainer.py:71-82
        o = dc.out
        gd = E.View.alloc(o.N, o.H, o.W, 1, dev) if train else None
        if kind_g is None:
            E.loss_value_and_grad(o, None, 1.0, L.LOSS_BCE, 1.0, gd, losses, 1, Bglobal)      # trainer.py:84
        else:
            E.gan_loss([(o, kind_g, 1.0, 1.0, gd, 1)], losses, Bglobal)                       # (the generator's target is never smoothed)
        g_reducer, late_adam_g = None, False
        self._mark('D(fake) fwd + losses done')
        if train:
            gflat = G.ensure_grad_flat()
            ddin = de.backward(dw, None, dc, gd, need_wgrad=False, need_dx=True, ucache=ucache)       # dL/d(x|gen)
            dgen = ddin.channels(Cin, Cout)
            if aug is not None:
                # D read T(x | G(x)): the gradient returns to G's output through the adjoint, into a view of its own
                dgen = E.diffaug_bwd(dgen, E.View.alloc(N, H, W, Cout, dev), aug_params, 0)
            self._mark('D dgrad done')
            if dist.on:
                # buckets of the flat G gradient are all-reduced on RCCL's stream as backward finishes them; the
                # collective keeps running under the discriminator step below (which does not read G's new weights:
                # gen_img.detach() is the pre-update output, trainer.py:98)
                # (two-stream step: a bucket's weight gradients may sit on the second stream -- the collective waits for it as well)
                g_reducer = GradReducer(dist, gflat, self.bucket_bytes, producers=E.side_producers)
            # two-stream step: G's weight gradients may still be running on the second stream when the pass returns; the
            # discriminator's forward below needs neither them nor G's new weights (gen_img.detach() is the pre-update output,
            # trainer.py:98), so the join and G's Adam update come after it
            two = bool(ex.enabled)
            late_adam_g = two and g_reducer is None
            ge.backward(G.flat, gflat, gc, gseg, dgen,                                        # trainer.py:88-89
                        on_ready=g_reducer.ready if g_reducer is not None else None, ucache=gcache, defer_join=two)
            ge.ucache_end(gcache)
            self._mark('G bwd (main chain) done')
            if late_adam_g:
                pass
            elif g_reducer is None:
                self._adam_step('g')                                                          # trainer.py:90
            else:
                g_reducer.finish(launch_only=True)     # the last (first layers') bucket leaves as soon as backward has produced it
        del dc

        # ---- discriminator step: real and (pre-update, detached) fake in one 2N batch        trainer.py:96-99
        if shared is not None:
            if not real_done:
                de.forward_part(dw, shared, 0, N, ucache=ucache)                              # trainer.py:96-97
            dc2 = shared
        elif dc2 is None:
            dc2 = de.forward(dw, din_d, ucache=ucache, keep_v=train, bn=D.bn_run(1, 2))
        if ex.pending or ex.keep:
            E.side_join()
        D.bn_update(3)        # BatchNorm discriminator in training mode: the three passes' updates in the reference's order (on this stream, after the join)
        self._mark('joined')
        capturing = self._adam_dev is not None      # (a step being captured ends with every chain joined: nothing is deferred across its end)
        adam_g_behind_fork = bool(train and late_adam_g and ex.enabled and E.PROFILER is None and DEFER_D_BWD and ADAM_G_BESIDE and not capturing)
        if train and late_adam_g and not adam_g_behind_fork:
            self._adam_step('g')                                                              # trainer.py:90
        o2 = dc2.out
        god = E.View.alloc(o2.N, o2.H, o2.W, 1, dev) if train else None
        if kind_d is None:
            E.loss_value_and_grad(o2.samples(0, N), None, real_label, L.LOSS_BCE, 0.5, god.samples(0, N) if train else None,
                                  losses, 2, Bglobal)                                         # loss_real
            E.loss_value_and_grad(o2.samples(N, N), None, 0.0, L.LOSS_BCE, 0.5, god.samples(N, N) if train else None,
                                  losses, 3, Bglobal)                                         # loss_fake
        else:
            # loss_real and loss_fake, the two sample halves of the one 2N map, as two terms of ONE launch
            E.gan_loss([(o2.samples(0, N), kind_d, real_label, 0.5, god.samples(0, N) if train else None, 2),
                        (o2.samples(N, N), kind_d, 0.0, 0.5, god.samples(N, N) if train else None, 3)], losses, Bglobal)
        wait_losses = None
        if dist.on:
            # the step's loss scalars for logging: seg is already global for tversky, the BCE / MAE terms are per-rank partial
            # means.  Summed on the comm stream under the discriminator's backward pass, ahead of its gradient all-reduce.
            if self.loss_type == 'tversky':
                losses[0] /= dist.world
            wait_losses = dist.all_reduce_side(losses)
        if train:
            dflat = D.ensure_grad_flat()
            if ex.enabled and E.PROFILER is None and DEFER_D_BWD and (g_reducer is None or DEFER_D_BWD_DP) and not capturing:
                # two-stream step: the discriminator's whole backward pass and its Adam update go to the second stream and run under the
                # NEXT step's generator forward, which reads neither D's weights nor its gradients (trainer.py:63; the next use of D is
                # trainer.py:66) and has no second chain of its own -- the same kernels with the same arguments, so the results are
                # bit-identical; flush() joins before anything reads D's weights (the next step's D passes, save / load, the end of train,
                # state_dict() / forward of the module).  The pass's operands stay referenced until then.
                with E.on_side():
                    de.backward(dw, dflat, dc2, god, need_wgrad=True, need_dx=False, ucache=ucache)       # trainer.py:106
                    if g_reducer is not None:
                        self._pending_d = dist.all_reduce_side(dflat)      # (behind the pass on the second stream; Adam(D) in flush())
                        self._pending_d_acc = self._acc_cur
                    else:
                        self._adam_step('d')                                                      # trainer.py:107
                    self._mark('side: D bwd done')
                self._deferred = (ex, dc2, god, ucache, dflat)
                if adam_g_behind_fork:
                    # G's Adam update (1.2 GB at the memory rate, 0.2 ms alone on the chip) beside the first kernels of D's backward pass
                    # instead of in front of them: it only has to precede the next step's generator forward
                    self._adam_step('g')                                                          # trainer.py:90
                if g_reducer is not None:
                    self._mark('forked')
                    g_reducer.finish()                     # G's buckets have been in flight since the generator backward
                    self._mark('G buckets waited')
                    self._adam_step('g')
                    self._mark('Adam(G) done')
            else:
                de.backward(dw, dflat, dc2, god, need_wgrad=True, need_dx=False, ucache=ucache)       # trainer.py:106
                if g_reducer is not None:
                    # D's gradient (11 MB at ndf=64) is all-reduced asynchronously and applied by flush() at the first use of
                    # D's weights -- after the NEXT step's generator forward, which does not read them (trainer.py:63-66); handed to
                    # the comm stream BEFORE the compute stream waits for G's buckets, so it is queued behind them without a gap
                    self._pending_d = dist.all_reduce_side(dflat)
                    self._pending_d_acc = self._acc_cur
                    g_reducer.finish()                     # G's buckets have been in flight since the generator backward
                    self._adam_step('g')
                else:
                    self._adam_step('d')                                                          # trainer.py:107
        de.ucache_end(ucache)
        if wait_losses is not None:
            wait_losses()
        self._mark('end')
        self._last_gen = gen
        return losses

    def _publish(self, losses):
        # the step's one device-to-host copy, asynchronous into a pinned slot: the returned dict waits for it on first access
        ring = getattr(self, '_loss_ring', None)
        if ring is None or ring[0][0].device != torch.device('cpu'):
            ring = self._loss_ring = [[torch.empty(4, dtype=torch.float32).pin_memory(), None] for _ in range(4)]
            self._loss_slot = 0
        slot = ring[self._loss_slot]
        self._loss_slot = (self._loss_slot + 1) % len(ring)
        if slot[1] is not None:
            slot[1]._fill()                # a result four steps old that nobody read yet: take its values out of the slot first
        slot[0].copy_(losses, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        slot[1] = out = StepLosses(slot[0], ev)
        return out

    def flush(self):
        """Complete a discriminator update that is still in flight: under data parallelism its gradient all-reduce (Adam(D) is applied
        here), in a two-stream step the backward pass + Adam(D) running on the second stream under the next generator forward.  Called
        before anything reads the discriminator's weights: the next step's D passes, save(), load(), the end of train(), and -- through
        the modules' access hook -- state_dict() / forward() / .to() of the discriminator itself."""
        if self._deferred is not None:
            ex = self._deferred[0]          # the execution state the pass was enqueued on (self._exec may have been replaced since)
            if ex is not None and (ex.pending or ex.keep):
                with ex:
                    E.side_join()
            self._deferred = None
        wait = getattr(self, '_pending_d', None)
        if wait is not None:
            self._pending_d = None
            wait()
            # (accumulate: with the place in the window of the call that made this gradient, not of the call that completes it)
            self._adam_step('d', acc=self._pending_d_acc)

    _ACC_CUR = object()

    def _adam_step(self, which, acc=_ACC_CUR):
        """Network `which`'s optimizer update on its flat gradient, on the current stream.  With `accumulate` set this is where the
        gradient joins its window instead: `acc` = (phase, gradients in the window with this one), by default the place of the training
        call being enqueued; only a closing phase goes on to the update, on the window's mean gradient."""
        o = self._opt(which)
        net = o.net
        if acc is Trainer._ACC_CUR:
            acc = self._acc_cur
        if which == 'd' and net.engine.spectral:
            # the passes ran on W / sigma: the flat gradient (all-reduced already under data parallelism -- the map is linear in it, and
            # u, v, sigma agree on every rank) becomes the gradient of the stored weights, on this stream, ahead of the norm and Adam
            # (accumulate: every call's gradient on its own, ahead of the sum -- call i ran on W / sigma_i; not once more for a window
            #  closed by step_accumulated(), whose accumulator holds mapped gradients)
            if acc is None or acc[0] != 'close_only':
                net.spectral_grad_map(net.grad_flat)
        if acc is not None:
            phase, count = acc
            E.grad_accum(o.acc, net.grad_flat, phase, E.accum_scale(count))
            self._acc_launches += 1       # (an enqueued accumulate launch is a commitment of the step, as an update is: batch())
            if phase in ('begin', 'add'):
                return            # weights, moments, the weight average and the step count stay as they are
        stat = None
        if o.max_norm is not None:
            # the norm of the whole flat gradient (two short launches) and Adam on g * coef, both behind the gradient on this stream;
            # a non-finite norm skips the update on the device -- the host's step count advances regardless
            self._clip_ensure()
            stat = self._clip_stat(which)
            E.grad_norm(net.grad_flat, o.max_norm, self._clip[1 + o.i], stat)
        # One fused pass (engine.adam_update picks the entry point): the decoupled decay, the clipping coefficient and the generator's
        # weight average ride in the Adam kernel where they are set.  A step being captured reads lr / bc1, sqrt(bc2) and the decay
        # multiplier from device memory (written before every replay, _replay, which also advances the step counts); otherwise this
        # launch is step o.t + 1 and the count advances here.
        if o.scal is not None:
            when = dict(scalars=o.scal)
        else:
            when = dict(step=o.t + 1, lr=o.lr)
            self._t_g, self._t_d = self._t_g + (1 - o.i), self._t_d + o.i
        E.adam_update(net.flat, net.grad_flat, o.m, o.v, ema=o.ema, ema_decay=o.ema_decay, stat=stat, weight_decay=o.weight_decay,
                      beta1=o.betas[0], beta2=o.betas[1], **when)

    # -------------------------------------------------------------------------------------- how a step is launched
    def _graph_eligible(self):
        """Capture applies: single GPU, dropout off (its per-layer seeds are launch arguments derived from the step number on the
        host), and no launch profiler armed (its HIP events are per launch: the HIP runtime torch brings along refuses external
        event-record nodes inside a capture, tools/graph_event_probe.py)."""
        G = self.generator
        if not self.graph or os.environ.get('PATCHGAN_GRAPH', '1') == '0' or _dist().on or E.PROFILER is not None:
            return False
        return not (G.training and G.engine.use_dropout)

    def _two_streams_setting(self):
        ts = self.two_streams
        if ts is None:
            ts = 'auto' if self.graph == 'auto' else False
        if E.PROFILER is not None or E._exp_env('PATCHGAN_TWO_STREAMS') == '0':
            return False          # (the launch profiler's event pairs keep everything on one stream)
        if _dist().on and (self.generator.engine.sync_bn or self.discriminator.engine.sync_bn):
            return False          # (SyncBatchNorm's per-layer collectives are issued from ONE compute stream, in one order on every rank)
        return ts

    def _kind_key(self, x, y, u8, dims, train):
        # (the max-norms are launch arguments of pg_grad_norm, as the decay is one of Adam(G): a captured step holds the values it was
        #  captured with, a changed value is another kind of step.  Off: the key is the one without the feature)
        clip = self._clip_now() if train else (None, None)
        # (likewise the augmentation's policy and seed, launch arguments of pg_diffaug_params)
        aug = self._aug_now() if train else None
        return (self._kind_key_base(x, y, u8, dims, train) + ((clip,) if clip != (None, None) else ())
                + ((('diffaug',) + aug,) if aug is not None else ()) + (self._optim_key() if train else ())
                + (self._acc_key() if train else ()))

    def _kind_key_base(self, x, y, u8, dims, train):
        G, D = self.generator, self.discriminator
        return (bool(train), u8, dims, self.loss_type, float(self.seg_alpha), float(self.tversky_beta), float(self.tversky_gamma),
                tuple(self.label_values) if self.label_values is not None else None, G.training, D.training,
                G.engine.algo, bool(G.engine.act_bf), D.engine.algo, bool(D.engine.act_bf), G.flat.data_ptr(), D.flat.data_ptr(),
                tuple(x.shape), tuple(y.shape), x.dtype, y.dtype, _dist().on,
                self._ema_now(),          # (the decay is a launch argument of Adam(G): a captured step holds the value it was captured with)
                # (an evaluation step with the metrics launch is another kind of step than one without: never timed against each other)
                # (likewise one with the histogram launch of metric_bins)
                ((float(self.metric_threshold), self.metric_bins) if self.metric_bins is not None else float(self.metric_threshold))
                if (self.metrics and not train) else None) + self._gan_key() + self._seg_key()

    def _seg_key(self):
        # (the term mask and the three settings are launch arguments of the new objectives' kernels: a captured step holds what it was
        #  captured with.  One of the reference's three: the key is the one without the feature, whatever the settings hold)
        spec = self._seg_now()
        return (('seg',) + tuple(spec),) if spec is not None else ()

    def _gan_key(self):
        # (the objective's kinds, targets and scales are launch arguments: a captured step holds what it was captured with.  The
        #  default: the key is the one without the feature)
        gan = self._gan_now()
        return (gan,) if gan != ('vanilla', 1.0, 'sigmoid') else ()

    def _launch_mode(self, key, train):
        """'eager1' (launch by launch, one stream) | 'eager2' (launch by launch, two streams) | 'graph' (replay) for this step of kind
        `key`.  What the settings allow is re-read every step (a profiler armed later, a group initialised later); what was measured
        is remembered per kind."""
        want_graph = self.graph if (train and self._graph_eligible()) else False
        ts = self._two_streams_setting()
        if key in self._oom_kinds:
            ts = False                            # (did not fit in device memory: _two_stream_oom)
        if not want_graph and not ts:
            return 'eager1'
        if ts is True and want_graph is not True:
            return 'eager2'                       # forced: no warm-up needed (entries a pass makes on the second stream are joined, _enqueue_step)
        k = self._kinds.pop(key, None) or {'seen': 0, 'mode': None, 'trial': None}
        self._kinds[key] = k                      # most recently used last
        while len(self._kinds) > self.MAX_KINDS:
            self._kinds.pop(next(iter(self._kinds)))
        if k['mode'] is not None:
            if (k['mode'] in ('graph', 'graph2') and not want_graph) or (k['mode'] in ('eager2', 'graph2') and not ts):
                return 'eager1'
            return k['mode']
        k['seen'] += 1
        if want_graph is True:                    # capture, no questions: after the warm steps
            if k['seen'] <= self.GRAPH_WARM_STEPS:
                return 'eager1'
            k['mode'] = 'graph'
            return 'graph'
        cands = ['eager1'] + (['eager2'] if ts else []) + (['graph'] if want_graph else [])
        forced = os.environ.get('PATCHGAN_AUTO_FORCE') if 'PATCHGAN_EXPERIMENT' in os.environ else None
        forced = forced or self.AUTO_FORCE
        if forced is not None:                    # by decree (tests, A/B runs): after the warm steps, no trials
            if k['seen'] <= self.GRAPH_WARM_STEPS:
                return 'eager1'
            k['mode'] = forced if (forced in cands or (forced == 'graph2' and 'graph' in cands and 'eager2' in cands)) else 'eager1'
            return k['mode']
        if k['seen'] == 1:
            return 'eager1'                       # untimed: kernel plans, weight-cache plans, workspaces
        tr = k['trial']
        if tr is None or tr['cands'] != cands:    # (the settings changed under a running tournament, or a step raised: start over)
            tr = k['trial'] = {'cands': cands, 'i': 0, 'starts': [], 'at': [], 'ms': {}, 'host': {}, 'step': -1}
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()                               # the start of this step on the compute stream
        if self._acc_cur is None:
            apart = tr['step'] != self._step - 1
        else:
            # accumulate: the phases of a window are kinds of their own that follow each other call by call and go through their
            # candidates together, so a period from one 'begin' to the next is a window launched one way; it scores per call (the
            # division below).  Only a step from outside the run of windows (_acc_run: since which step) breaks a period.
            apart = self._acc_run is None or tr['step'] < self._acc_run[1]
        if tr['starts'] and apart:
            # a step of ANOTHER kind ran since this kind's last one (validation batches, a ragged last batch, an evaluation pass): the
            # period would span it -- this candidate's trial starts over
            tr['starts'], tr['at'] = [], []
        tr['step'] = self._step
        tr['starts'].append(ev)
        tr['at'].append(self._step)
        if len(tr['starts']) <= 2 * self.TRIAL_STEPS + 1:
            return tr['cands'][tr['i']]
        # 2 x TRIAL_STEPS + 1 starts of this candidate and the start of the step that follows them: its periods are known once that last
        # event has been reached (one wait per candidate, during warm-up).  The first TRIAL_STEPS periods do not score: they hold the
        # switch and the caching allocator's growth for the new launch pattern (a second stream allocates from a pool of its own:
        # device allocations synchronise -- seen at 2-3 x the settled step time for the first steps)
        ev.synchronize()
        st, at = tr['starts'], tr['at']
        tr['ms'][tr['cands'][tr['i']]] = min(st[j].elapsed_time(st[j + 1]) / (at[j + 1] - at[j]) for j in range(self.TRIAL_STEPS, len(st) - 1))
        tr['i'] += 1
        tr['starts'], tr['at'] = [ev], [self._step]
        if tr['i'] < len(cands) and cands[tr['i']] == 'graph' and tr['ms']['eager1'] > self.GRAPH_TRIAL_RATIO * tr['host'].get('eager1', 0.0):
            # a replay removes host time only: where the one-stream step is well clear of being host-bound the capture (which would
            # hold a second copy of the step's activations, ~4 GB at cfg2) cannot win and is not tried
            tr['ms']['graph'] = None
            tr['i'] += 1
        if tr['i'] < len(cands):
            return cands[tr['i']]
        dist = _dist()
        if dist.on:
            # every rank keeps the same way of launching: the slowest rank's time per candidate decides (ranks reach this point at the
            # same step: trials and their restarts depend on the step sequence only)
            dev = self.generator.flat.device
            t = torch.tensor([tr['ms'][m] if tr['ms'][m] is not None else 1e30 for m in cands], dtype=torch.float64,
                             device=dev if dist.backend == 'nccl' else 'cpu')
            dist.dist.all_reduce(t, op=dist.dist.ReduceOp.MAX)
            for m, v in zip(cands, t.tolist()):
                if tr['ms'][m] is not None:
                    tr['ms'][m] = v
        self.step_times = dict(tr['ms'], host_enqueue=dict(tr['host']))
        k['mode'] = min((m for m in cands if tr['ms'][m] is not None), key=lambda m: tr['ms'][m])
        k['trial'] = None
        for two in (False, True):                 # the losing captures' buffers go back to the allocator
            if k['mode'] != ('graph2' if two else 'graph'):
                self._graphs.pop((key, two), None)
        return k['mode']

    def _two_stream_oom(self, ex, key):
        """A two-stream step ran out of device memory before anything was committed: join and drop the second stream's state, give the
        workspaces and the allocator's cache back, and pin this kind of step to one stream (redecide() forgets the pin)."""
        import warnings
        ex.enabled = False
        try:
            E.side_join()
        except Exception:
            pass
        torch.cuda.synchronize(ex.device)
        self._deferred = None
        ex.release()
        torch.cuda.empty_cache()
        self._oom_kinds.add(key)
        k = self._kinds.get(key)
        if k is not None:
            k['mode'], k['trial'] = 'eager1', None
        self.oom_fallbacks += 1
        warnings.warn('patchgan_amd: the two-stream step ran out of device memory (it holds about twice what the one-stream step '
                      'does: INTEGRATION.md, "Memory"); this kind of step runs on one stream from here on')

    def __del__(self):
        # a discriminator update still running on the second stream references this trainer's tensors: join before they are freed
        try:
            if self._deferred is not None:
                self.flush()
        except Exception:
            pass

    def redecide(self):
        """Forget every launch decision and captured step (the next steps of each kind warm up, are timed and decided again)."""
        self.flush()
        self._kinds, self._graphs = {}, {}
        self._oom_kinds = set()

    def release(self):
        """Give this trainer's captured steps, workspaces and second stream back (they also go with the object)."""
        self.flush()
        self._graphs = {}
        if self._exec is not None:
            self._exec.release()

    def _replay(self, key, x, y, u8, dims, two=False):
        """The training step replayed from a captured hipGraph: ~220 launches become one hipGraphLaunch (host enqueue 1.9 ms -> well
        under 0.1 ms per step at cfg2; the step itself is unchanged -- same kernels, same arguments, bit-identical results).
        Captured on first use.  Per replay the host copies the inputs into the graph's input buffers, writes Adam's two
        step-dependent scalars per network (lr / bc1, sqrt(bc2): pg_adam_step_dev reads them from device memory; with a weight decay
        set a third, the decay multiplier of the step's learning rate: pg_adamw_step_dev) and launches.
        Returns None (after a warning) if this runtime cannot capture the step: the caller continues launch by launch."""
        self.flush()
        key = (key, bool(two))            # (a kind's one-stream and two-stream captures are different graphs)
        st = self._graphs.get(key)
        if st is not None and st.ptrs != self._graph_ptrs():
            # the gradient / moment buffers the capture was made with were replaced (a network moved, .grad reset): capture again
            del self._graphs[key]
            st = None
        if st is None:
            try:
                st = self._capture(key, x, y, u8, dims, two)
            except Exception as e:          # a runtime that cannot capture this step: launch by launch from here on, loudly
                import warnings
                warnings.warn(f'patchgan_amd: hipGraph capture of the training step failed ({type(e).__name__}: {e}); continuing launch by launch')
                self.graph = False
                return None
        else:
            self._graphs[key] = self._graphs.pop(key)          # most recently used last
        st.x.copy_(x, non_blocking=True)
        st.y.copy_(y, non_blocking=True)
        if self._acc_cur is None or self._acc_cur[0] == 'close':
            # (accumulate: only the graph of a window's closing call holds Adam launches -- the others move no step count and read no scalars)
            self._t_g += 1
            self._t_d += 1
            host = st.host[st.slot]
            st.slot = (st.slot + 1) % len(st.host)
            h = host.numpy()
            k = st.scal.numel() // 2
            for i, which in enumerate('gd'):
                h[i * k:(i + 1) * k] = self._adam_scalars(which, k)
            st.scal.copy_(host, non_blocking=True)
        st.graph.replay()
        self._last_gen = st.gen
        self._aug_params = st.aug_params
        return st.losses

    def _graph_ptrs(self):
        G, D = self.generator, self.discriminator
        return tuple(t.data_ptr() if t is not None else 0 for t in (G.grad_flat, D.grad_flat) + self._opt_buffers())

    def _capture(self, key, x, y, u8, dims, two=False):
        class _StepGraph:
            pass
        st = _StepGraph()
        dev = x.device
        G, D = self.generator, self.discriminator
        st.x, st.y = torch.empty_like(x), torch.empty_like(y)
        # (lr / bc1 and sqrt(bc2) per network; with a weight decay set for either, three floats per network: + the decay multiplier)
        nscal = 6 if self._optim_now()[1] != (None, None) else 4
        st.scal = torch.zeros(nscal, dtype=torch.float32, device=dev)
        # (a ring: the copy of slot i to the device may still be queued when the host prepares the next steps; _publish's ring of
        #  four loss slots keeps the host at most four steps ahead of the device)
        st.host, st.slot = [torch.zeros(nscal, dtype=torch.float32).pin_memory() for _ in range(8)], 0
        # (accumulate: the phases of one window are graphs of their own and follow each other call by call -- room for all of them)
        room = self.MAX_GRAPHS if self._acc_cur is None else max(self.MAX_GRAPHS, min(self._acc_k, 3))
        while len(self._graphs) >= room:
            self._graphs.pop(next(iter(self._graphs)))
        G.ensure_grad_flat()
        D.ensure_grad_flat()
        st.graph = torch.cuda.CUDAGraph()
        self._adam_dev = st.scal
        ex = E.cur_exec(dev)
        try:
            # two: the fork / join schedule of the two-stream step inside the capture -- the second stream joins the capture through the
            # events the engine already uses (stream waits become graph dependencies) and every chain it runs is joined again before the
            # step ends; the one piece that crosses the step boundary, the discriminator's deferred backward pass, stays inside the step
            ex.enabled = bool(two)
            with torch.cuda.graph(st.graph, capture_error_mode='thread_local'):
                st.losses = self._enqueue_step(st.x, st.y, u8, *dims, True)
                if two and (ex.pending or ex.keep):
                    E.side_join()
                st.gen = self._last_gen
                st.aug_params = self._aug_params if self._aug_now() is not None else None
        finally:
            ex.enabled = False
            self._adam_dev = None
        # The graph has baked in the addresses of buffers it does not own: the workspace(s), the transformed / packed weight entries of
        # both networks, the flat gradients and Adam's moments.  It keeps every one of them alive -- a workspace that grows for a larger
        # extent, a weight-cache pool cleared by set_precision / set_tuning or trimmed by its plan limit replace THEIR reference, not this
        # one, so a replay never writes into memory the allocator has handed to someone else -- and it is captured again if the
        # buffers whose CONTENT matters outside the graph (gradients, moments) were replaced (_graph_ptrs).
        st.hold = (E.cur_exec(dev).buffers() + list(G.engine.__dict__.get('_upool', {}).values())
                   + list(D.engine.__dict__.get('_upool', {}).values()) + [G.grad_flat, D.grad_flat]
                   + [t for t in self._opt_buffers() if t is not None]
                   + ([D.sn_bufs, D.sn_eff] + list(D.sn_ws) if D.engine.spectral else [])
                   + ([self._aug_counter] if st.aug_params is not None else []))
        seg_spec = self._seg_now()
        if seg_spec is not None and seg_spec.cw is not None:
            st.hold.append(seg_spec.cw)      # (class_weights: the buffer the captured loss launch reads)
        st.ptrs = self._graph_ptrs()
        self._graphs[key] = st
        return st

    def graph_captured(self):
        """True once some kind of training step runs from a captured graph (bench.py warms up until then)."""
        return bool(self._graphs)

    def graph_decided(self):
        """True once a kind of step has been captured or its launch mode decided ('auto')."""
        return bool(self._graphs) or any(k['mode'] is not None for k in self._kinds.values())

    def decided_modes(self):
        """The launch modes decided so far, one per kind of step, most recently used last ('eager1' | 'eager2' | 'graph')."""
        return [k['mode'] for k in self._kinds.values() if k['mode'] is not None]

    # -------------------------------------------------------------------------------------- epoch driver
    def train(self, train_data, val_data, epochs, dsc_learning_rate=1.e-3, gen_learning_rate=1.e-3, save_freq=10,
              lr_decay=None, decay_freq=5, reduce_on_plateau=False):
        """Reference trainer.py:117-279: Adam(lr, betas=(0.9, 0.999)) for G and D, optional exponential LR decay every
        `decay_freq` epochs (resumed as lr*decay^((start-1)/decay_freq)), per-epoch train + validation loops, checkpoint
        every `save_freq` epochs.  Returns (G_loss_ep, D_loss_ep): per-epoch means of the training losses.
        With `metrics` the validation pass also yields IoU / Dice (val_history, one printed line per epoch) and `save_best` keeps the
        best epoch's weights (_validated)."""
        if self.save_best is not None:
            if not self.metrics:
                raise ValueError(f"Trainer.save_best = {self.save_best!r} needs Trainer.metrics = True (the score comes from the validation counts)")
            if self._best is None or self._best.metric != self.save_best:
                self._best = BestTracker(self.save_best)      # (a resumed run keeps what load_last_checkpoint() read back)
        self._metric_bins()      # (ValueError for a bin count pg_seg_hist does not take, or one without `metrics`)
        if isinstance(self.class_weights, str):
            # a scheme name that nothing has resolved yet: the estimate, on the training data, before the first epoch
            scheme = self.class_weights
            ge = self.generator.engine
            if E.check_seg_loss(self.loss_type, ge.final_act, ge.output_nc, self.focal_gamma, self.focal_alpha, self.dice_smooth) is None:
                self._seg_now()      # (one of the reference's three objectives has no per-class weights: ValueError before any pass over the data)
            self.estimate_class_weights(train_data, scheme, self.class_weight_batches)
            if _dist().rank == 0:
                info = self.class_weight_info
                print(f"Class weights ({scheme}) -- counts: {info['counts']}  unlabelled: {info['unlabelled']} of {info['pixels']} "
                      f"pixels  weights: {[round(w, 4) for w in info['weights']]}")
        if (lr_decay is not None) and not reduce_on_plateau:
            gen_lr = gen_learning_rate * (lr_decay) ** ((self.start - 1) / (decay_freq))
            dsc_lr = dsc_learning_rate * (lr_decay) ** ((self.start - 1) / (decay_freq))
        else:
            gen_lr, dsc_lr = gen_learning_rate, dsc_learning_rate

        if self.neptune_config is not None:
            self.neptune_config['model/parameters/gen_learning_rate'] = gen_lr
            self.neptune_config['model/parameters/dsc_learning_rate'] = dsc_lr
            self.neptune_config['model/parameters/start'] = self.start
            self.neptune_config['model/parameters/n_epochs'] = epochs

        self.setup_optimizers(gen_lr, dsc_lr)
        plateau = None
        if reduce_on_plateau:
            plateau = [_Plateau(gen_lr), _Plateau(dsc_lr)]
            if self._resume_plateau is not None:
                # a resumed run (save_optimizer): the schedule goes on from its saved learning rates, best values and patience counts
                for pl, saved in zip(plateau, self._resume_plateau):
                    pl.lr, pl.best, pl.bad = float(saved['lr']), float(saved['best']), int(saved['bad'])
                self.gen_lr, self.dsc_lr = plateau[0].lr, plateau[1].lr
            if self.neptune_config is not None:
                self.neptune_config['model/parameters/scheduler'] = 'ReduceLROnPlateau'
        elif lr_decay is not None and self.neptune_config is not None:
            self.neptune_config['model/parameters/scheduler'] = 'ExponentialLR'
            self.neptune_config['model/parameters/decay_freq'] = decay_freq
            self.neptune_config['model/parameters/lr_decay'] = lr_decay

        self._plateau, self._resume_plateau = plateau, None
        history = {'gen': [], 'disc': []}
        try:
            return self._epochs(train_data, val_data, epochs, save_freq, lr_decay, decay_freq, plateau, history)
        finally:
            # also on an exception / KeyboardInterrupt inside the loop.  gc.unfreeze() is process-global: it also thaws what the host
            # application froze itself (which is why gc_freeze is opt-in)
            self._plateau = None
            if self.gc_freeze:
                _unsettle_gc()

    def _epochs(self, train_data, val_data, epochs, save_freq, lr_decay, decay_freq, plateau, history):
        for epoch in range(self.start, epochs + 1):
            if _dist().rank == 0:
                print(f"Epoch {epoch} -- lr: {self.gen_lr:5.3e}, {self.dsc_lr:5.3e}")
                print("-------------------------------------------------------")
            calls0, updates0 = self._acc_calls, self._acc_updates
            train_mean = self._run_epoch(train_data, True, epoch, 'Training: ', dynamic_ncols=True)
            if self._acc_now() is not None:
                # a window the epoch's last batches left open is closed short (its mean over what it holds): validation, the schedule
                # and the checkpoint below never see half a window
                self.step_accumulated()
                if _dist().rank == 0:
                    print(f"Accumulation -- {self._acc_updates - updates0} optimizer steps from {self._acc_calls - calls0} "
                          f"micro-batches (accumulate = {self._acc_now()})")
            for key in history:
                history[key].append(train_mean[key])
            if self._clip_now() != (None, None):
                self._grad_stats_epoch(epoch)
            # the reference keeps ONE running-mean dict across both loops: a validation pass without batches reports the
            # training means (trainer.py:204-262)
            if self.metrics:
                self.reset_metrics()
            val_mean = dict(train_mean, **self._run_epoch(val_data, False, epoch, 'Validation: '))
            if self.neptune_config is not None:
                for phase, mean in (('train', train_mean), ('eval', val_mean)):
                    self.neptune_config[f'{phase}/gen_loss'].append(mean['gen'])
                    self.neptune_config[f'{phase}/disc_loss'].append(mean['disc'])
            if self.metrics:
                self._validated(epoch, val_mean, val_data)

            if plateau is not None:
                self.gen_lr = plateau[0].step(val_mean['gen'])
                self.dsc_lr = plateau[1].step(val_mean['disc'])
            elif lr_decay is not None and epoch % decay_freq == 0:
                self.gen_lr *= lr_decay        # ExponentialLR.step() (trainer.py:266-270)
                self.dsc_lr *= lr_decay

            if epoch % save_freq == 0:
                self.save(epoch)
        self.flush()
        return history['gen'], history['disc']

    def _grad_stats_epoch(self, epoch):
        """After an epoch's training loop with `clip_grad_norm`: the one host read of the status blocks, one printed line, reset."""
        stats = self.read_grad_stats()
        self.grad_history.append(dict({'epoch': epoch}, **stats))
        self.reset_grad_stats()
        if _dist().rank == 0:
            def line(s):
                return (f"mean {s['mean_norm']:.4g}  max {s['max_norm']:.4g}  clipped {s['clipped']}/{s['steps']}"
                        f"  skipped {s['skipped']}")
            print(f"Gradient norm -- generator: {line(stats['gen'])}  |  discriminator: {line(stats['disc'])}")

    def _validated(self, epoch, val_mean, val_data):
        """After an epoch's validation pass with `metrics`: read its counts (a collective under data parallelism, as is the averaged
        generator's own pass), record and print the scores, and keep the best weights so far (save_best)."""
        live = self.read_metrics()
        entry = dict({'epoch': epoch}, **{k: val_mean[k] for k in StepLosses.KEYS if k in val_mean})
        entry.update({k: v for k, v in live.items() if k not in CURVE_ONLY})
        ema = None
        if self.ema_generator is not None:
            ema = self.evaluate(val_data, self.ema_generator)
            entry['ema'] = {k: v for k, v in ema.items() if k not in CURVE_ONLY}
        self.val_history.append(entry)
        rank0 = _dist().rank == 0
        if rank0:
            def line(s):
                text = f"mIoU {s['miou']:.4f}  mDice {s['mdice']:.4f}  pixel acc {s['pixel_acc']:.4f}"
                if 'mean_ap' in s:          # (metric_bins; several channels: the first class that has a best threshold)
                    ok = np.flatnonzero(~np.isnan(s['best_threshold']))
                    c = int(ok[0]) if ok.size else 0
                    text += (f"  mean AP {s['mean_ap']:.4f}  best threshold {s['best_threshold'][c]:.4f}"
                             + (f" (class {c})" if len(s['best_threshold']) > 1 else "") + f" with IoU {s['best_iou'][c]:.4f}")
                return text
            print(f"Validation metrics -- {line(live)}" + (f"  |  averaged generator: {line(ema)}" if ema is not None else ""))
        if self.neptune_config is not None:
            self.neptune_config['eval/miou'].append(live['miou'])
            self.neptune_config['eval/mdice'].append(live['mdice'])
        if self.save_best is None:
            return
        # (the scores come from all-reduced integers: every rank takes the same decision; rank 0 writes)
        better = self._best.update('generator', epoch, live)
        better_ema = ema is not None and self._best.update('generator_ema', epoch, ema)
        if not (better or better_ema):
            return
        self.flush()
        if not rank0:
            return
        if better:
            print(f"Best {self.save_best} so far ({live[self.save_best]:.4f}): saving to {self.savefolder}best_generator.pth and best_discriminator.pth")
            torch.save(self.generator.state_dict_contiguous(), f'{self.savefolder}/best_generator.pth')
            torch.save(self.discriminator.state_dict_contiguous(), f'{self.savefolder}/best_discriminator.pth')
        if better_ema:
            print(f"Best {self.save_best} of the averaged generator so far ({ema[self.save_best]:.4f}): saving to {self.savefolder}best_generator_ema.pth")
            torch.save(self.ema_generator.state_dict_contiguous(), f'{self.savefolder}/best_generator_ema.pth')
        self._best.save(self.savefolder)

    def _run_epoch(self, data, train, epoch, desc, **bar_kwargs):
        """One pass over `data` through batch(train=...): networks switched to train() / eval(), the data source
        reshuffled (a `shuffle()` method as the reference calls it, trainer.py:206,236, or a DistributedSampler's
        set_epoch under data parallelism), running means of the six loss scalars shown on the progress bar.
        Returns {key: mean over the pass}."""
        for net in (self.generator, self.discriminator):
            net.train(train)
        bar = tqdm.tqdm(data, desc=desc, disable=_dist().rank != 0, **bar_kwargs)
        if hasattr(data, 'shuffle'):
            data.shuffle()
        sampler = getattr(data, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)           # otherwise every epoch repeats the first permutation / rank shards
        sums, count, mean = defaultdict(float), 0, {}

        def account(step_losses):
            nonlocal count, mean
            count += 1
            for key, value in step_losses.items():          # (waits for that step's device-to-host copy)
                sums[key] += value
            mean = {key: total / count for key, total in sums.items()}
            bar.set_postfix_str(" ".join(f"{key}: {value:.2e}" for key, value in mean.items()))

        pending = None          # the bar shows step i once step i + 1 is enqueued: the GPU never waits for the logging
        for input_img, target_mask in bar:
            cur = self.batch(input_img, target_mask, train=train)
            if pending is not None:
                account(pending)
            pending = cur
        if pending is not None:
            account(pending)
        return mean

    # -------------------------------------------------------------------------------------- checkpoints
    def save(self, epoch):
        """generator_ep_%03d.pth / discriminator_ep_%03d.pth holding torch-layout state_dicts (trainer.py:281-287)."""
        self.flush()
        if _dist().rank != 0:
            return
        gen_savefile = f'{self.savefolder}/generator_ep_{epoch:03d}.pth'
        disc_savefile = f'{self.savefolder}/discriminator_ep_{epoch:03d}.pth'
        print(f"Saving to {gen_savefile} and {disc_savefile}")
        torch.save(self.generator.state_dict_contiguous(), gen_savefile)
        torch.save(self.discriminator.state_dict_contiguous(), disc_savefile)
        if self.ema_generator is not None:
            # the averaged generator: the same keys and shapes as generator_ep_*.pth, so anything that loads one loads the other
            # (patchgan_infer's checkpoint_paths.generator); the name stays clear of load_last_checkpoint's generator_ep*.pth glob
            ema_savefile = f'{self.savefolder}/generator_ema_ep_{epoch:03d}.pth'
            print(f"Saving to {ema_savefile}")
            torch.save(self.ema_generator.state_dict_contiguous(), ema_savefile)
        if self.save_optimizer:
            # Adam's moments and step counts and the trainer's own counters, for an exact resume; the name stays clear of the two globs
            opt_savefile = f'{self.savefolder}/optimizer_ep_{epoch:03d}.pth'
            print(f"Saving to {opt_savefile}")
            torch.save(self.optimizer_state(epoch), opt_savefile)

    def optimizer_state(self, epoch=None):
        """What save() writes to optimizer_ep_%03d.pth with save_optimizer set: {'format': 1, 'gen', 'disc', 'trainer'}.  'gen' and
        'disc' are state_dicts that torch.optim.Adam(list(net.parameters())) -- AdamW where weight_decay is set -- loads as they are
        (optimizer_section); 'trainer' holds epoch, gen_lr, dsc_lr, t_g, t_d, step (the host step number the dropout seeds derive
        from), diffaug_counter (the device word, read here; None without one) and plateau (the two schedules' lr / best / bad inside
        train(reduce_on_plateau=True), else None).  CPU tensors.  Completes a discriminator update in flight."""
        self.flush()
        def section(o):
            # (nothing trained yet: zero moments at step 0, what a fresh optimizer starts from)
            m, v = (o.m, o.v) if o.m is not None else (torch.zeros_like(o.net.flat), torch.zeros_like(o.net.flat))
            return optimizer_section(o.net, m, v, o.t, o.lr, o.betas, o.weight_decay)
        plateau = self._plateau
        return {
            'format': 1,
            'gen': section(self._opt('g')),
            'disc': section(self._opt('d')),
            'trainer': {
                'epoch': epoch, 'gen_lr': float(self.gen_lr), 'dsc_lr': float(self.dsc_lr), 't_g': int(self._t_g), 't_d': int(self._t_d),
                'step': int(self._step),
                'diffaug_counter': int(self._aug_counter.cpu()[0]) if self._aug_counter is not None else None,
                'plateau': [dict(lr=float(pl.lr), best=float(pl.best), bad=int(pl.bad)) for pl in plateau] if plateau is not None else None,
            },
        }

    def load_optimizer_state(self, path):
        """Read an optimizer_ep_*.pth (or the dict optimizer_state() returns): its 'gen' / 'disc' sections may also come straight from
        the state_dict() of a torch.optim.Adam / AdamW over the modules' parameters; 'trainer' may be missing.  RuntimeError for a wrong
        parameter count or shape.  The state is PENDING: the next setup_optimizers() -- train() calls it, as does the first training
        batch() of a trainer without optimizers -- takes it over instead of starting fresh."""
        sd = torch.load(path, map_location='cpu') if not isinstance(path, dict) else path
        if not isinstance(sd, dict) or 'gen' not in sd or 'disc' not in sd:
            raise RuntimeError(f"{path if not isinstance(path, dict) else 'the given dict'}: not an optimizer state of this trainer (no 'gen' / 'disc' sections)")
        if sd.get('format', 1) != 1:
            raise RuntimeError(f"optimizer state of format {sd.get('format')!r}: this version reads format 1")
        G, D = self.generator, self.discriminator
        gm, gv, dm, dv = (torch.zeros(G.flat.numel()), torch.zeros(G.flat.numel()), torch.zeros(D.flat.numel()), torch.zeros(D.flat.numel()))
        t_g = load_optimizer_section(G, sd['gen'], gm, gv, 'gen')
        t_d = load_optimizer_section(D, sd['disc'], dm, dv, 'disc')
        tr = sd.get('trainer')
        if tr is not None:
            t_g, t_d = int(tr.get('t_g', t_g)), int(tr.get('t_d', t_d))
        self._resume = {'adam': (gm, gv, dm, dv), 't_g': t_g, 't_d': t_d, 'trainer': dict(tr) if tr is not None else None}

    def load_last_checkpoint(self):
        gen_ck = sorted(glob.glob(self.savefolder + "generator_ep*.pth"))
        dsc_ck = sorted(glob.glob(self.savefolder + "discriminator_ep*.pth"))
        gen_epochs = set(int(os.path.basename(c).replace('generator_ep_', '')[:-4]) for c in gen_ck)
        dsc_epochs = set(int(os.path.basename(c).replace('discriminator_ep_', '')[:-4]) for c in dsc_ck)
        try:
            self._class_weights_restore()      # (class_weights = a scheme name: the estimate an earlier run left in the folder)
            assert len(gen_epochs) > 0, "No checkpoints found!"
            start = max(gen_epochs.union(dsc_epochs))
            ema_save = f"{self.savefolder}/generator_ema_ep_{start:03d}.pth"
            self.load(f"{self.savefolder}/generator_ep_{start:03d}.pth", f"{self.savefolder}/discriminator_ep_{start:03d}.pth",
                      ema_save if os.path.exists(ema_save) else None)
            self.start = start + 1
            if self.save_optimizer:
                opt_save = f"{self.savefolder}/optimizer_ep_{start:03d}.pth"
                if os.path.exists(opt_save):
                    self.load_optimizer_state(opt_save)
                    print(f"Loaded the optimizer state from {os.path.basename(opt_save)}")
                else:
                    print(f"No {os.path.basename(opt_save)}: the optimizers start fresh")
            best = BestTracker.load(self.savefolder)      # (save_best: the resumed run competes with the best model already on disk)
            if best is not None:
                self._best = best
        except Exception as e:
            print(e)
            print("Checkpoints not loaded")

    def load(self, generator_save, discriminator_save, ema_save=None):
        """With ema_decay set, the weight average comes from `ema_save` (a generator_ema_ep_*.pth); without such a file it
        restarts from the generator weights just loaded."""
        self.flush()
        self._acc_done = 0        # (accumulate: an open window's gradients belong to the weights that are replaced here)
        print(generator_save, discriminator_save)
        dev = self.generator.flat.device
        self.generator.load_state_dict(torch.load(generator_save, map_location=dev))
        self.discriminator.load_state_dict(torch.load(discriminator_save, map_location=dev))
        print(f"Loaded checkpoints from {os.path.basename(generator_save)} and {os.path.basename(discriminator_save)}")
        if self.ema_decay is not None:
            self.reset_ema()
            if ema_save is None:
                print("No averaged-generator checkpoint given: the weight average restarts from the loaded generator weights")
            else:
                # (parameters only: a BatchNorm generator's running statistics are the live generator's tensors, loaded above)
                sd = torch.load(ema_save, map_location=dev)
                own = self._ema_net.state_dict()
                if set(sd) != set(own):
                    raise RuntimeError(f"{ema_save}: not a state_dict of this generator")
                with torch.no_grad():
                    for k, _ in self._ema_net.named_parameters():
                        own[k].copy_(sd[k])
                print(f"Loaded the weight average from {os.path.basename(ema_save)}")


def optimizer_section(net, m, v, step, lr, betas=(0.9, 0.999), weight_decay=None):
    """The state_dict of a torch.optim.Adam (AdamW with a weight_decay) over list(net.parameters()) that has taken `step` steps with
    the flat moment buffers `m`, `v` of `net` (a UNet / Discriminator of this package): state[i] = {step: float32 scalar, exp_avg,
    exp_avg_sq}, i in net.parameters() order, every tensor in the parameter's own shape, contiguous, on the CPU; one param_groups
    entry.  The views are engine.torch_views of the moment buffers: the mechanism that makes the parameters views of net.flat."""
    names = [k for k, _ in net.named_parameters()]
    mv, vv = E.torch_views(m.detach(), net._layers), E.torch_views(v.detach(), net._layers)
    state = {i: {'step': torch.tensor(float(step), dtype=torch.float32), 'exp_avg': mv[k].contiguous().cpu().clone(),
                 'exp_avg_sq': vv[k].contiguous().cpu().clone()} for i, k in enumerate(names)}
    group = {'lr': float(lr), 'betas': (float(betas[0]), float(betas[1])), 'eps': 1e-8, 'weight_decay': float(weight_decay or 0.0),
             'amsgrad': False, 'params': list(range(len(names)))}
    return {'state': state, 'param_groups': [group]}


def load_optimizer_section(net, section, m, v, name='optimizer'):
    """The reverse of optimizer_section: fill the flat moment buffers `m`, `v` (in net.flat's layout) from `section` -- one written by
    optimizer_section or the state_dict() of a torch optimizer over list(net.parameters()) -- and return its step count.  A parameter
    without a state entry (it never had a gradient) keeps zero moments.  RuntimeError for a wrong parameter count or shape."""
    names = [k for k, _ in net.named_parameters()]
    try:
        state, groups = section['state'], section['param_groups']
        ids = [i for g in groups for i in g['params']]
    except (KeyError, TypeError):
        raise RuntimeError(f"{name}: not an optimizer state_dict (state / param_groups)") from None
    if len(ids) != len(names) or any(i not in ids for i in state):
        raise RuntimeError(f"{name}: the optimizer state holds {len(ids)} parameters, the network has {len(names)}")
    mv, vv = E.torch_views(m, net._layers), E.torch_views(v, net._layers)
    step = 0
    with torch.no_grad():
        for i, k in zip(ids, names):
            st = state.get(i)
            if st is None:
                continue
            for key, views in (('exp_avg', mv), ('exp_avg_sq', vv)):
                if tuple(st[key].shape) != tuple(views[k].shape):
                    raise RuntimeError(f"{name}: {key} of parameter {i} ({k}) has shape {tuple(st[key].shape)}, the network's is {tuple(views[k].shape)}")
            mv[k].copy_(st['exp_avg'])
            vv[k].copy_(st['exp_avg_sq'])
            step = max(step, int(float(st['step'])))
    return step


class _Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau with its defaults, as the reference constructs it (trainer.py:175-178: mode
    'min', factor 0.1, patience 10, relative threshold 1e-4, cooldown 0, min_lr 0, eps 1e-8), on a scalar learning rate:
    step(metric) after every epoch (trainer.py:271-273) returns the learning rate for the next one.
    tests/test_trainer_cpu.py holds it against torch's class."""

    def __init__(self, lr):
        self.lr, self.best, self.bad = lr, float('inf'), 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1 - 1e-4):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > 10:
            new_lr = max(self.lr * 0.1, 0.0)
            if self.lr - new_lr > 1e-8:        # torch ignores updates smaller than eps
                self.lr = new_lr
            self.bad = 0
        return self.lr
