"""``patchgan_infer`` -- tiled inference (reference patchgan/infer.py:14-174) with the generator forward on the HIP path.

``predict_image`` is what ``patchgan_infer`` runs per image: ``pg_tiles_gather`` (image -> NHWC tile batch), the generator
forward, ``pg_tiles_blend`` (overlap average in float64, optional threshold, class argmax) -- three stages of HIP kernels
with no layout conversion in between.  ``n_crop`` / ``build_mask`` keep the reference's function signatures (NCHW tensors in
and out, any device) for user code that calls them directly.  The reference indexes tiles with ``j * ncropsy + i``
(infer.py:32,57), which is only correct for square images (it overwrites / skips tiles otherwise); here the row-major
index ``j * ncropsx + i`` is used, identical for square images and correct for the rest.

Beyond the reference: ``tta`` (flipped / transposed variants of every tile as further samples, ``pg_tiles_gather_tta``) and ``window``
(a separable blend window that down-weights tile borders, ``pg_tiles_blend_win``).  Both default to ``None``, which is the reference's
uniform average over one forward per tile, through the same launches as before.
"""
import argparse
import os

import numpy as np
import torch
import tqdm
import yaml

from .disc import Discriminator
from .io import COCOStuffDataset, load_plugin_dataset
from .unet import UNet


def _starts(extent, size, eff):
    n = int(np.ceil(extent / eff))
    out = []
    for k in range(n):
        s = k * eff
        s -= max(s + size - extent, 0)
        out.append(s)
    return out


def _tta_apply(x, k):
    """Variant k of a [..., size, size] tile: transpose(-1, -2) if k & 4, then flip(-2) if k & 2, then flip(-1) if k & 1."""
    if k & 4:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-2)
    if k & 1:
        x = x.flip(-1)
    return x


def _tta_undo(x, k):
    """The inverse of _tta_apply: the same steps undone in reverse order."""
    if k & 1:
        x = x.flip(-1)
    if k & 2:
        x = x.flip(-2)
    if k & 4:
        x = x.transpose(-1, -2)
    return x


def n_crop(image, size, overlap, tta=None):
    """tta ('hflip' / 'flips' / 'd4'): K = 2 / 4 / 8 variants of every tile; variant k of tile t is crops[k * T + t]."""
    c, height, width = image.shape
    eff = int(overlap * size)
    ys, xs = _starts(height, size, eff), _starts(width, size, eff)
    if tta is not None:
        from .engine import tta_variants
        ntiles = len(xs) * len(ys)
        crops = torch.zeros((tta_variants(tta) * ntiles, c, size, size), device=image.device)
        for k in range(tta_variants(tta)):
            for j, sy in enumerate(ys):
                for i, sx in enumerate(xs):
                    crops[k * ntiles + j * len(xs) + i] = _tta_apply(image[:, sy:sy + size, sx:sx + size], k)
        return crops
    crops = torch.zeros((len(xs) * len(ys), c, size, size), device=image.device)
    for j, sy in enumerate(ys):
        for i, sx in enumerate(xs):
            crops[j * len(xs) + i] = image[:, sy:sy + size, sx:sx + size]
    return crops


def _build_mask_weighted(masks, crop_size, image_size, threshold, overlap, tta, window):
    """build_mask with test-time augmentation and / or a blend window -- the arithmetic of pg_tiles_blend_win restated in torch:
    tiles in row-major order, the K variants of a tile in order, every product and sum in float64 and rounded on its own."""
    from .engine import tta_variants, window_table
    nvar = tta_variants(tta)
    n, c, height, width = masks.shape
    ih, iw = image_size
    dev = masks.device
    win = torch.from_numpy(window_table(window, crop_size)).to(dev)
    mask = torch.zeros((c, ih, iw), dtype=torch.float64, device=dev)
    wsum = torch.zeros((c, ih, iw), dtype=torch.float64, device=dev)
    eff = int(overlap * crop_size)
    ys, xs = _starts(ih, crop_size, eff), _starts(iw, crop_size, eff)
    ntiles = len(xs) * len(ys)
    if n != nvar * ntiles:
        raise ValueError(f"{n} tiles do not tile a {ih}x{iw} image with overlap {overlap} in {nvar} variants")
    wgt = win[:, None] * win[None, :]
    for j, sy in enumerate(ys):
        for i, sx in enumerate(xs):
            for k in range(nvar):
                term = wgt * _tta_undo(masks[k * ntiles + j * len(xs) + i], k).double()
                mask[:, sy:sy + crop_size, sx:sx + crop_size] += term
                wsum[:, sy:sy + crop_size, sx:sx + crop_size] += wgt
    return mask / wsum


def build_mask(masks, crop_size, image_size, threshold, overlap, tta=None, window=None):
    masks = torch.as_tensor(masks)
    n, c, height, width = masks.shape
    ih, iw = image_size
    dev = masks.device
    if tta is not None or window is not None:
        mask = _build_mask_weighted(masks, crop_size, image_size, threshold, overlap, tta, window)
    else:
        mask = torch.zeros((c, ih, iw), dtype=torch.float64, device=dev)
        count = torch.zeros((c, ih, iw), dtype=torch.float64, device=dev)
        eff = int(overlap * crop_size)
        ys, xs = _starts(ih, crop_size, eff), _starts(iw, crop_size, eff)
        for j, sy in enumerate(ys):
            for i, sx in enumerate(xs):
                mask[:, sy:sy + crop_size, sx:sx + crop_size] += masks[j * len(xs) + i].double()
                count[:, sy:sy + crop_size, sx:sx + crop_size] += 1
        mask = mask / count
    if threshold > 0:
        mask = (mask >= threshold).double()
    mask = mask.cpu().numpy()
    if c > 1:
        return np.argmax(mask, axis=0)
    return mask[0]


def predict_image(generator, image, size, overlap, threshold, max_tiles=None, tta=None, window=None):
    """One image [C, H, W] (device tensor) -> mask as numpy: float64 [H, W] for a single-class generator, class index
    [H, W] otherwise -- reference infer.py:155-163 (n_crop -> generator -> build_mask) on the HIP path end to end.
    The tiles STREAM through the generator at most `max_tiles` per forward pass (default: 64 tiles of 256 x 256, scaled with the
    tile area; tiles are independent samples, so the result does not depend on it): a 1024 x 1024 image (25 tiles) is one pass, a
    4096 x 4096 one (324 tiles) six -- activation memory and every tensor's byte extent stay bounded whatever the image size.
    tta: test-time augmentation, None / 'hflip' / 'flips' / 'd4' -- 1 / 2 / 4 / 8 flipped and transposed variants of every tile go through
    the generator as further samples, and the blend averages their predictions mapped back.  window: None (uniform average), 'pyramid',
    'hann' or `size` positive weights -- a separable window that down-weights tile borders in the blend (engine.window_table)."""
    from . import engine as E
    eng = generator.engine
    E.tta_variants(tta)
    if window is not None:
        E.window_table(window, size)          # ValueError before any launch
    if eng.has_bn and generator.training:
        # batch statistics would depend on how the tiles are grouped into passes (max_tiles); the reference's patchgan_infer
        # always calls .eval()
        raise ValueError("predict_image: a BatchNorm2d generator in training mode would normalise each pass of tiles with its own "
                         "batch statistics -- call generator.eval() first (the running statistics are used then)")
    tiles = E.tiles_gather(image, size, overlap, tta)
    pred = E.View.alloc(tiles.N, size, size, eng.output_nc, image.device)
    if max_tiles is None:
        max_tiles = max(1, (64 * 256 * 256) // (size * size))
    for t0 in range(0, tiles.N, max_tiles):
        n = min(max_tiles, tiles.N - t0)
        eng.forward(generator.flat, tiles.samples(t0, n), pred.samples(t0, n), False, 0, bn=generator.bn_run())
    mask = E.tiles_blend(pred, tuple(image.shape[1:]), threshold, overlap, tta, window)
    # device -> host through a pinned block of torch's caching host allocator (the numpy array keeps it alive; it returns to the cache when
    # the caller drops the mask): a pageable .cpu() of the 8-MB float64 mask took 0.3-1.2 ms of the 3-ms image, this one 0.15
    host = torch.empty(mask.shape, dtype=mask.dtype, pin_memory=True)
    host.copy_(mask, non_blocking=True)
    torch.cuda.current_stream(mask.device).synchronize()
    return host.numpy()


def patchgan_infer(argv=None):
    parser = argparse.ArgumentParser(prog='PatchGAN', description='Run PatchGAN inference')
    parser.add_argument('-c', '--config_file', required=True, type=str, help='Location of the config YAML file')
    parser.add_argument('--dataloader_workers', default=4, type=int)
    parser.add_argument('-d', '--device', default='auto', help='Device to use (CUDA=GPU)')
    parser.add_argument('--summary', default=True, action='store_true', help="Print summary of the models")
    args = parser.parse_args(argv)
    if args.device == 'cpu' or not torch.cuda.is_available():
        raise RuntimeError("patchgan_amd runs on a HIP device only (MI355X)")
    device = 'cuda'
    print(f"Running with {device}")

    with open(args.config_file, 'r') as infile:
        config = yaml.safe_load(infile)
    dataset_params = config['dataset']
    dataset_path = dataset_params['dataset_path']
    size = dataset_params.get('size', 256)
    dataset_kwargs = {}
    if dataset_params['type'] == 'COCOStuff':
        Dataset = COCOStuffDataset
        in_channels = 3
        labels = dataset_params.get('labels', [1])
        out_channels = len(labels)
        dataset_kwargs['labels'] = labels
    else:
        Dataset = load_plugin_dataset(dataset_params['type'])
        in_channels = dataset_params.get('in_channels', 3)
        out_channels = dataset_params.get('out_channels', 1)
    assert hasattr(Dataset, 'get_filename') and callable(Dataset.get_filename), \
        f"Dataset class {Dataset.__name__} must have the get_filename method which returns the image filename for a given index"
    assert hasattr(Dataset, 'save_mask') and callable(Dataset.save_mask), \
        f"Dataset class {Dataset.__name__} must have the save_mask method to save a mask cube for a given filename"
    datagen = Dataset(dataset_path, **dataset_kwargs)

    from .train import model_cfgs, norm_layer_of, print_summary, spectral_norm_of
    gen_cfg, disc_cfg = model_cfgs(config['model_params'])      # (the norm layers the checkpoints were trained with: train.NORM_LAYERS)
    generator = UNet(in_channels, out_channels, gen_cfg['filters'], activation=gen_cfg['activation'],
                     final_act=gen_cfg.get('final_activation', 'sigmoid'), norm_layer=norm_layer_of(gen_cfg.get('norm_layer'))).to(device)
    discriminator = Discriminator(in_channels + out_channels, disc_cfg['filters'], n_layers=disc_cfg['n_layers'],
                                  norm=disc_cfg.get('norm', False), norm_layer=norm_layer_of(disc_cfg.get('norm_layer')),
                                  spectral_norm=spectral_norm_of(disc_cfg.get('spectral_norm'))).to(device)
    if args.summary:
        print_summary('generator', generator)

    ck = config['checkpoint_paths']
    infer_params = config.get('infer_params', {})
    threshold = infer_params.get('threshold', 0)
    if isinstance(threshold, str):
        # `threshold: best` -- the threshold with the best validation IoU of exactly these weights, as train() stored it in
        # best_metrics.json beside best_generator*.pth (Trainer.metric_bins); ValueError before anything is written or processed
        if threshold != 'best':
            raise ValueError(f"infer_params.threshold must be a number or 'best', not {threshold!r}")
        from .metrics import best_threshold
        threshold = best_threshold(ck['generator'], out_channels)
        print(f"threshold: best = {threshold} (from best_metrics.json beside {os.path.basename(ck['generator'])})")
    output_path = infer_params.get('output_path', 'predictions/')
    if not os.path.exists(output_path):
        os.makedirs(output_path)
        print(f"Created folder {output_path}")
    generator.eval()
    discriminator.eval()
    generator.load_state_dict(torch.load(ck['generator'], map_location=device))
    discriminator.load_state_dict(torch.load(ck['discriminator'], map_location=device))
    overlap =infer_params.get('overlap', 0.9)
    tta = infer_params.get('tta')                 # absent: no test-time augmentation, uniform blend
    window = infer_params.get('window')           # a name or a list of `size` weights

    for i, data in enumerate(tqdm.tqdm(datagen, desc='Predicting', dynamic_ncols=True, ascii=True)):
        data = torch.as_tensor(data).to(device)
        out_fname, _ = os.path.splitext(datagen.get_filename(i))
        mask = predict_image(generator, data, size, overlap, threshold, tta=tta, window=window)
        Dataset.save_mask(mask, output_path, out_fname)


if __name__ == '__main__':
    patchgan_infer()
