"""``patchgan_train`` -- the reference's training CLI (patchgan/train.py:13-127) on the MI355X path.

Same flags (-c/--config_file, -b/--batch_size, --dataloader_workers, -n/--n_epochs, -d/--device, --summary) and the
same YAML keys.  Both config schemas are accepted: the one train.py v0.2.2 reads (``dataset.{train_data,validation_data}``
or ``dataset.{data,train_val_split}``, nested ``model_params.{generator,discriminator}``) and the older flat one that
``examples/train_coco.yaml`` and infer.py still use (top-level ``train_data`` / ``validation_data``,
``model_params.{gen_filts,disc_filts,n_disc_layers,activation,use_dropout,final_activation}``).

Extension: ``model_params.generator.norm_layer`` / ``model_params.discriminator.norm_layer`` (flat schema: ``gen_norm_layer`` /
``disc_norm_layer``) name the networks' norm layer: ``instance`` (the default), ``instance_affine``, ``batch`` or ``sync_batch``
(NORM_LAYERS); ``patchgan_infer`` reads the same keys to build the network a checkpoint was trained with.

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m patchgan_amd.train ...``; each rank
takes a distinct shard of every epoch (DistributedSampler) and gradients are all-reduced over RCCL.
"""
import argparse
import functools
import os

import numpy as np
import torch
import yaml
from torch import nn
from torch.utils.data import DataLoader, random_split

from .disc import Discriminator
from .io import COCOStuffDataset, load_plugin_dataset
from .trainer import Trainer
from .unet import UNet


NORM_LAYERS = {'instance': nn.InstanceNorm2d, 'instance_affine': functools.partial(nn.InstanceNorm2d, affine=True),
               'batch': nn.BatchNorm2d, 'sync_batch': nn.SyncBatchNorm}


def norm_layer_of(name='instance'):
    """The norm_layer constructor argument a YAML norm-layer value names (None, the key absent: 'instance'); ValueError otherwise."""
    name = 'instance' if name is None else name
    if not isinstance(name, str) or name not in NORM_LAYERS:
        raise ValueError(f"norm_layer must be one of {' | '.join(NORM_LAYERS)}, not {name!r}")
    return NORM_LAYERS[name]


def spectral_norm_of(value=None):
    """The spectral_norm constructor argument of the discriminator from its YAML value (None, the key absent: False); ValueError for
    anything but a bool."""
    value = False if value is None else value
    if not isinstance(value, bool):
        raise ValueError(f"spectral_norm must be true or false, not {value!r}")
    return value


def disc_final_act_of(value=None):
    """The final_act constructor argument of the discriminator from its YAML value (None, the key absent: 'sigmoid'); ValueError for
    anything but sigmoid | none."""
    from . import engine as E
    value = 'sigmoid' if value is None else value
    if not isinstance(value, str) or value not in E.DISC_FINAL_ACTS:
        raise ValueError(f"the discriminator's final_act must be one of {' | '.join(E.DISC_FINAL_ACTS)}, not {value!r}")
    return value


def gan_mode_of(mode=None, real_label=None, final_act='sigmoid'):
    """(Trainer.gan_mode, Trainer.real_label) from the YAML's train_params.gan_mode (vanilla | lsgan | hinge; absent = vanilla) and
    train_params.real_label (a number in (0, 1]; absent = 1), checked against the discriminator's final_act as Trainer.batch checks
    them.  ValueError for anything else, before any network is built."""
    from . import engine as E
    return E.check_gan_mode('vanilla' if mode is None else mode, 1.0 if real_label is None else real_label, final_act)


def optimizer_of(betas=None, weight_decay=None, save_optimizer=None, lrs=None):
    """(Trainer.betas, Trainer.weight_decay, Trainer.save_optimizer) from the YAML's train_params.betas -- a two-element list
    [beta1, beta2] for both networks or a mapping {gen: [..], disc: [..]} (a missing member: Adam's (0.9, 0.999)) --,
    train_params.weight_decay -- a number or a two-element list [generator, discriminator] whose members may be null -- and
    train_params.save_optimizer (true | false); absent = off.  With `lrs` = (gen, disc) the decay is also held against the learning
    rates (lr * weight_decay < 1).  ValueError for anything else, before any network is built."""
    from . import engine as E
    if isinstance(betas, dict):
        if not betas or set(betas) - {'gen', 'disc'}:
            raise ValueError(f"betas must be a list [beta1, beta2] or a mapping with the keys gen / disc, not {betas!r}")
        betas = tuple(tuple(b) if isinstance(b, list) else ((0.9, 0.999) if b is None else b)
                      for b in (betas.get('gen'), betas.get('disc')))
    elif isinstance(betas, list):
        betas = tuple(tuple(b) if isinstance(b, list) else b for b in betas)
    weight_decay = tuple(weight_decay) if isinstance(weight_decay, list) else weight_decay
    E.check_betas(betas)
    wd = E.check_weight_decay(weight_decay)
    if lrs is not None:
        for lr, w in zip(lrs, wd):
            if w is not None:
                E.decay_mul(lr, w)
    if save_optimizer is not None and not isinstance(save_optimizer, bool):
        raise ValueError(f"save_optimizer must be true or false, not {save_optimizer!r}")
    return betas, weight_decay, (True if save_optimizer else None)


def accumulate_of(value=None):
    """Trainer.accumulate from the YAML's train_params.accumulate: an int >= 2 = that many micro-batches per optimizer step; absent,
    null or 1 = off (None).  ValueError for anything else -- 0, a negative number, a float, true / false, a string --, before any
    network is built."""
    from . import engine as E
    return E.check_accumulate(value)


def _optimizer_of_params(tp):
    return optimizer_of(tp.get('betas', None), tp.get('weight_decay', None), tp.get('save_optimizer', None),
                        (tp.get('gen_learning_rate', 1e-3), tp.get('disc_learning_rate', 1e-3)))


def model_cfgs(mp):
    """(generator_cfg, disc_cfg) of either schema's model_params; a 'norm_layer' name, where one is given, is checked (norm_layer_of:
    ValueError before any network is built) and an absent one stays absent.  Likewise the discriminator's 'spectral_norm'
    (model_params.discriminator.spectral_norm, flat schema: disc_spectral_norm; spectral_norm_of) and its 'final_act'
    (model_params.discriminator.final_act, flat schema: disc_final_act; disc_final_act_of)."""
    if 'generator' in mp:
        gen_cfg, disc_cfg = dict(mp['generator']), dict(mp['discriminator'])
    else:                                                                         # flat legacy schema (infer.py:127-132)
        gen_cfg = {'filters': mp['gen_filts'], 'activation': mp['activation'],
                   'use_dropout': mp.get('use_dropout', True), 'final_activation': mp.get('final_activation', 'sigmoid')}
        disc_cfg = {'filters': mp['disc_filts'], 'n_layers': mp['n_disc_layers'], 'norm': mp.get('disc_norm', False)}
        for cfg, key in ((gen_cfg, 'gen_norm_layer'), (disc_cfg, 'disc_norm_layer')):
            if key in mp:
                cfg['norm_layer'] = mp[key]
        if 'disc_spectral_norm' in mp:
            disc_cfg['spectral_norm'] = mp['disc_spectral_norm']
        if 'disc_final_act' in mp:
            disc_cfg['final_act'] = mp['disc_final_act']
    for cfg in (gen_cfg, disc_cfg):
        norm_layer_of(cfg.get('norm_layer'))
    spectral_norm_of(disc_cfg.get('spectral_norm'))
    disc_final_act_of(disc_cfg.get('final_act'))
    return gen_cfg, disc_cfg


def parse_config(config):
    """Normalise either YAML schema into (dataset_params, train_paths, val_paths, split, generator_cfg, disc_cfg)."""
    dataset_params = dict(config['dataset'])
    for key in ('train_data', 'validation_data', 'data', 'train_val_split'):      # legacy: paths at top level
        if key not in dataset_params and key in config:
            dataset_params[key] = config[key]
    if ('train_data' in dataset_params) and ('validation_data' in dataset_params):
        train_paths, val_paths, split = dataset_params['train_data'], dataset_params['validation_data'], None
    elif ('data' in dataset_params) and ('train_val_split' in dataset_params):
        train_paths, val_paths, split = dataset_params['data'], None, dataset_params['train_val_split']
    else:
        raise AttributeError("Please provide either the training and validation data paths or a train/val split!")
    if 'labels' not in dataset_params and isinstance(train_paths, dict) and 'labels' in train_paths:
        dataset_params['labels'] = train_paths['labels']                          # legacy: labels next to the paths
    gen_cfg, disc_cfg = model_cfgs(config['model_params'])
    return dataset_params, train_paths, val_paths, split, gen_cfg, disc_cfg


def apply_train_params(trainer, train_params):
    """The trainer settings of the YAML's train_params: loss_type, seg_alpha and -- optional, absent = off -- ema_decay, the decay of
    the generator's weight average (Trainer.ema_decay; checkpoints then include generator_ema_ep_*.pth), metrics / metric_threshold
    (Trainer.metrics: per-epoch validation IoU / Dice from counts kept on the device), save_best ('miou' | 'mdice': best_*.pth),
    metric_bins (Trainer.metric_bins: a power of two in 16..1024 -- score curves, average precision and the best threshold) and
    clip_grad_norm (Trainer.clip_grad_norm: a number for both networks or a two-element list [generator, discriminator] whose members
    may be null; a non-finite gradient then skips the step), diffaug / diffaug_seed (Trainer.diffaug: differentiable augmentation of
    the discriminator's inputs; diffaug_of), gan_mode / real_label (Trainer.gan_mode: the adversarial objective; gan_mode_of), betas /
    weight_decay / save_optimizer (Trainer.betas, Trainer.weight_decay: Adam's betas and AdamW's decoupled decay per network;
    Trainer.save_optimizer: optimizer_ep_*.pth beside the checkpoints, for an exact resume; optimizer_of), accumulate
    (Trainer.accumulate: micro-batches per optimizer step; accumulate_of), focal_gamma / focal_alpha / dice_smooth (the settings of
    loss_type = 'ce' | 'focal' | 'dice' and their '+'-joined sums; seg_loss_of), class_weights / class_weight_batches
    (Trainer.class_weights: per-class weights of those objectives, a list or 'balanced' | 'balanced_sqrt'; class_weights_of)."""
    ge = trainer.generator.engine
    trainer.focal_gamma, trainer.focal_alpha, trainer.dice_smooth = seg_loss_of(train_params, ge.final_act, ge.output_nc)
    trainer.class_weights, trainer.class_weight_batches = class_weights_of(train_params, ge.final_act, ge.output_nc)
    trainer.loss_type = train_params['loss_type']
    trainer.seg_alpha = train_params['seg_alpha']
    trainer.ema_decay = train_params.get('ema_decay', None)
    clip = train_params.get('clip_grad_norm', None)
    trainer.clip_grad_norm = tuple(clip) if isinstance(clip, list) else clip
    trainer.metrics = True if train_params.get('metrics', None) else None
    trainer.metric_threshold = float(train_params.get('metric_threshold', 0.5))
    trainer.save_best = train_params.get('save_best', None)
    trainer.metric_bins = train_params.get('metric_bins', None)
    trainer.diffaug, trainer.diffaug_seed = diffaug_of(train_params.get('diffaug', None), train_params.get('diffaug_seed', None))
    trainer.gan_mode, trainer.real_label = gan_mode_of(train_params.get('gan_mode', None), train_params.get('real_label', None),
                                                       trainer.discriminator.final_act)
    trainer.betas, trainer.weight_decay, trainer.save_optimizer = _optimizer_of_params(train_params)
    trainer.accumulate = accumulate_of(train_params.get('accumulate', None))


def seg_loss_of(train_params, final_act, out_channels):
    """(Trainer.focal_gamma, Trainer.focal_alpha, Trainer.dice_smooth) from the YAML's train_params.focal_gamma (an integer in 0..8;
    absent = 2), focal_alpha (a number in (0, 1); absent or null = none) and dice_smooth (a finite number > 0; absent = 1), checked
    together with train_params.loss_type against the generator's head and channel count as Trainer.batch checks them
    (engine.check_seg_loss): ValueError.  With one of the reference's three loss types the settings are inert and not checked."""
    from . import engine as E
    from .trainer import Trainer
    gamma = train_params.get('focal_gamma', None)
    smooth = train_params.get('dice_smooth', None)
    out = (Trainer.focal_gamma if gamma is None else gamma, train_params.get('focal_alpha', None),
           Trainer.dice_smooth if smooth is None else smooth)
    E.check_seg_loss(train_params['loss_type'], final_act, out_channels, *out)
    return out


def class_weights_of(train_params, final_act, out_channels):
    """(Trainer.class_weights, Trainer.class_weight_batches) from the YAML's train_params.class_weights -- a list of one number per
    output channel (finite, >= 0, at least one > 0) or 'balanced' | 'balanced_sqrt' (estimated from the training masks before the first
    epoch); absent or null = off -- and train_params.class_weight_batches (how many training batches the estimate counts: an integer
    >= 1; absent or null = all).  Checked with the objective as Trainer.batch checks them (engine.check_seg_loss): ValueError, also
    for weights beside one of the reference's three loss types, which have none."""
    from . import engine as E
    from .trainer import Trainer
    cw = train_params.get('class_weights', None)
    nb = train_params.get('class_weight_batches', None)
    if nb is not None and (isinstance(nb, bool) or not isinstance(nb, int) or nb < 1):
        raise ValueError(f"class_weight_batches must be an integer >= 1, not {nb!r}")
    if cw is None:
        if nb is not None:
            raise ValueError("class_weight_batches needs class_weights = 'balanced' | 'balanced_sqrt'")
        return None, None
    gamma, smooth = train_params.get('focal_gamma', None), train_params.get('dice_smooth', None)
    settings = (Trainer.focal_gamma if gamma is None else gamma, train_params.get('focal_alpha', None),
                Trainer.dice_smooth if smooth is None else smooth)
    if isinstance(cw, str) and cw in E.CLASS_WEIGHT_SCHEMES:
        # (a scheme: the objective must be one that takes weights, on at least two channels; the values come from the data)
        if E.check_seg_loss(train_params['loss_type'], final_act, out_channels, *settings) is None:
            raise ValueError(f"class_weights = {cw!r} needs loss_type = {' | '.join(E.SEG_OBJECTIVES)} or a sum of them; loss_type = "
                             f"{train_params['loss_type']!r} has no per-class weights")
        if int(out_channels) < 2:
            raise ValueError(f"class_weights = {cw!r}: one output channel has nothing to be balanced against")
        return cw, nb
    if nb is not None:
        raise ValueError("class_weight_batches needs class_weights = 'balanced' | 'balanced_sqrt'")
    if isinstance(cw, tuple):
        cw = list(cw)
    E.check_seg_loss(train_params['loss_type'], final_act, out_channels, *settings, cw)
    return cw, None


def diffaug_of(policy=None, seed=None):
    """(Trainer.diffaug, Trainer.diffaug_seed) from the YAML's train_params.diffaug -- a comma-separated string or a list out of flip,
    translation, cutout; absent or empty = off -- and train_params.diffaug_seed (an int; absent = 0).  ValueError for anything else,
    before any batch is read."""
    from . import engine as E
    seed = E.diffaug_seed(0 if seed is None else seed)
    if policy is not None and not isinstance(policy, (str, list)):
        raise ValueError(f"diffaug must be a string or a list out of {', '.join(E.AUG_POLICIES)}, not {policy!r}")
    return (policy if E.diffaug_policy(policy) else None), seed


def print_summary(name, module):
    n = sum(p.numel() for p in module.parameters())
    print(f"{name}: {n:,} parameters in {len(list(module.parameters()))} tensors")
    for k, v in module.state_dict().items():
        print(f"  {k:48s} {tuple(v.shape)}")


def patchgan_train(argv=None):
    parser = argparse.ArgumentParser(prog='PatchGAN', description='Train the PatchGAN architecture')
    parser.add_argument('-c', '--config_file', required=True, type=str, help='Location of the config YAML file')
    parser.add_argument('-b', '--batch_size', default=16, type=int, help='Number of images per batch (per GPU)')
    parser.add_argument('--dataloader_workers', default=4, type=int,
                        help='Number of workers to use with dataloader (set to 0 to disable multithreading)')
    parser.add_argument('-n', '--n_epochs', required=True, type=int, help='Number of epochs to train the model')
    parser.add_argument('-d', '--device', default='auto', help='Device to use to train the model (CUDA=GPU)')
    parser.add_argument('--summary', default=True, action='store_true', help="Print summary of the models")
    args = parser.parse_args(argv)

    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.device == 'cpu' or not torch.cuda.is_available():
        raise RuntimeError("patchgan_amd trains on a HIP device only (MI355X); no GPU is visible / --device cpu requested")
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    if world > 1:
        import torch.distributed as dist
        import datetime
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        # bounded rendezvous / collective timeout: a rank whose peer died fails within minutes instead of holding its GPU for
        # the backend's 10-30 min default (torch.distributed.run then tears the job down)
        dist.init_process_group('nccl', device_id=device,
                                timeout=datetime.timedelta(seconds=float(os.environ.get('PATCHGAN_DIST_TIMEOUT_S', '600'))))

    with open(args.config_file, 'r') as infile:
        config = yaml.safe_load(infile)
    dataset_params, train_paths, val_paths, split, gen_cfg, disc_cfg = parse_config(config)
    # (the objective against the discriminator's head: a ValueError here, before any data set or network is built)
    gan_mode_of(config['train_params'].get('gan_mode'), config['train_params'].get('real_label'), disc_final_act_of(disc_cfg.get('final_act')))
    _optimizer_of_params(config['train_params'])      # (likewise the optimizer's settings)
    accumulate_of(config['train_params'].get('accumulate'))      # (likewise the accumulation window)
    # (likewise the segmentation objective, against the generator's head and the mask's channel count)
    seg_loss_of(config['train_params'], gen_cfg.get('final_activation', 'sigmoid'),
                len(dataset_params.get('labels', [1])) if dataset_params['type'] == 'COCOStuff' else dataset_params.get('out_channels', 1))
    # (likewise its per-class weights)
    class_weights_of(config['train_params'], gen_cfg.get('final_activation', 'sigmoid'),
                     len(dataset_params.get('labels', [1])) if dataset_params['type'] == 'COCOStuff' else dataset_params.get('out_channels', 1))

    size = dataset_params.get('size', 256)
    augmentation = dataset_params.get('augmentation', 'randomcrop')
    dataset_kwargs = {}
    if dataset_params['type'] == 'COCOStuff':
        Dataset = COCOStuffDataset
        in_channels = 3
        labels = dataset_params.get('labels', [1])
        out_channels = len(labels)
        dataset_kwargs['labels'] = labels
        if dataset_params.get('device_pipeline', False):      # extension: `/255.` + one-hot on the GPU (io.py docstring)
            dataset_kwargs['device_pipeline'] = True
    else:
        Dataset = load_plugin_dataset(dataset_params['type'])
        in_channels = dataset_params.get('in_channels', 3)
        out_channels = dataset_params.get('out_channels', 1)

    if split is None:
        train_datagen = Dataset(train_paths['images'], train_paths['masks'], size=size, augmentation=augmentation, **dataset_kwargs)
        val_datagen = Dataset(val_paths['images'], val_paths['masks'], size=size, augmentation=augmentation, **dataset_kwargs)
    else:
        datagen = Dataset(train_paths['images'], train_paths['masks'], size=size, augmentation=augmentation, **dataset_kwargs)
        train_datagen, val_datagen = random_split(datagen, split, generator=torch.Generator().manual_seed(0))

    dloader_kwargs = {}
    if args.dataloader_workers > 0:
        dloader_kwargs['num_workers'] = args.dataloader_workers
        dloader_kwargs['persistent_workers'] = True
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        train_data = DataLoader(train_datagen, batch_size=args.batch_size, pin_memory=True, drop_last=True,
                                sampler=DistributedSampler(train_datagen, shuffle=True), **dloader_kwargs)
        val_data = DataLoader(val_datagen, batch_size=args.batch_size, pin_memory=True, drop_last=True,
                              sampler=DistributedSampler(val_datagen, shuffle=False), **dloader_kwargs)
    else:
        train_data = DataLoader(train_datagen, batch_size=args.batch_size, shuffle=True, pin_memory=True, **dloader_kwargs)
        val_data = DataLoader(val_datagen, batch_size=args.batch_size, shuffle=True, pin_memory=True, **dloader_kwargs)

    generator = UNet(in_channels, out_channels, gen_cfg['filters'], use_dropout=gen_cfg.get('use_dropout', True),
                     activation=gen_cfg['activation'], final_act=gen_cfg.get('final_activation', 'sigmoid'),
                     norm_layer=norm_layer_of(gen_cfg.get('norm_layer'))).to(device)
    discriminator = Discriminator(in_channels + out_channels, disc_cfg['filters'], norm=disc_cfg.get('norm', False),
                                  n_layers=disc_cfg['n_layers'], norm_layer=norm_layer_of(disc_cfg.get('norm_layer')),
                                  spectral_norm=spectral_norm_of(disc_cfg.get('spectral_norm')),
                                  final_act=disc_final_act_of(disc_cfg.get('final_act'))).to(device)
    if world > 1:
        import torch.distributed as dist
        dist.broadcast(generator.flat, 0)          # every rank starts from rank 0's initial weights
        dist.broadcast(discriminator.flat, 0)
        if discriminator.spectral_norm:
            dist.broadcast(discriminator.sn_bufs, 0)      # ... and rank 0's u, v: the ranks' normalised weights stay equal bit for bit
    if args.summary and local_rank == 0:
        print_summary('generator', generator)
        print_summary('discriminator', discriminator)

    checkpoint_path = config.get('checkpoint_path', './checkpoints/')
    trainer = Trainer(generator, discriminator, savefolder=checkpoint_path)
    trainer.gc_freeze = True      # this process is the training job: keep generation-2 collections out of the step loop
    # per kind of step the trainer times two warm steps and decides: a launch-bound one is replayed from a captured hipGraph (one GPU,
    # use_dropout: False); a device-bound one stays launch by launch on two streams -- also with use_dropout: True (the default,
    # reference train.py:92), in the validation loop and under data parallelism
    trainer.graph = 'auto'
    if dataset_kwargs.get('device_pipeline', False):
        trainer.label_values = [int(v) for v in np.sort(dataset_kwargs['labels'])]
    train_params = config['train_params']
    apply_train_params(trainer, train_params)      # (before a resume: with ema_decay set, load() restores the weight average too)
    if config.get('load_last_checkpoint', False):
        trainer.load_last_checkpoint()
    elif config.get('transfer_learn', {}).get('generator_checkpoint', None) is not None:
        gen_checkpoint = config['transfer_learn']['generator_checkpoint']
        dsc_checkpoint = config['transfer_learn']['discriminator_checkpoint']
        generator.load_transfer_data(torch.load(gen_checkpoint, map_location=device))
        discriminator.load_transfer_data(torch.load(dsc_checkpoint, map_location=device))

    return trainer.train(train_data, val_data, args.n_epochs,
                         dsc_learning_rate=train_params['disc_learning_rate'],
                         gen_learning_rate=train_params['gen_learning_rate'],
                         lr_decay=train_params.get('decay_rate', None),
                         save_freq=train_params.get('save_freq', 10))


if __name__ == '__main__':
    patchgan_train()
