"""N-layer PatchGAN discriminator with the reference's surface (patchgan/disc.py:5-51) on gfx950 kernels."""
import torch
from torch import nn

from . import engine as E
from ._module import FlatParamModule
from .transfer import Transferable


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        eng = module.engine
        N, C, H, W = x.shape
        dev = module.flat.device
        din = E.View.alloc(N, H, W, C, dev).from_nchw(x.to(device=dev, dtype=torch.float32))
        flat = module.flat
        ctx.sn = None
        if eng.spectral:
            # torch's hook: one power iteration per training-mode call, none in eval mode.  This call's normalised weights, u, v and
            # sigma are kept for its backward pass (a later forward overwrites the module's own)
            flat = module.spectral_normalize().clone()
            ctx.sn = module.sn_bufs.clone()
        c = eng.forward(flat, din, bn=module.bn_run())
        module.bn_update(1)          # training mode: this call's batch statistics into the running statistics, as torch does
        ctx.module, ctx.c, ctx.flat = module, c, flat
        ctx.need_dx = x.requires_grad
        return c.out.to_nchw()

    @staticmethod
    def backward(ctx, gout):
        module, c = ctx.module, ctx.c
        eng = module.engine
        o = c.out
        g = E.View.alloc(o.N, o.H, o.W, 1, module.flat.device).from_nchw(gout.to(torch.float32))
        gflat = torch.zeros_like(module.flat)
        dx = eng.backward(ctx.flat, gflat, c, g, need_wgrad=True, need_dx=ctx.need_dx)
        if ctx.sn is not None:
            module.spectral_grad_map(gflat, ctx.flat, ctx.sn)
        views = E.torch_views(gflat, eng.layers)
        grads = tuple(views[k] for k in module._param_keys)
        return (None, dx.to_nchw() if dx is not None else None) + grads


class Discriminator(FlatParamModule, Transferable):
    """Discriminator(input_nc, ndf=64, n_layers=3, norm=False, norm_layer=InstanceNorm2d, spectral_norm=False, final_act='sigmoid') --
    reference disc.py:8.
    norm_layer: nn.InstanceNorm2d, nn.BatchNorm2d or -- for data parallelism: the global batch's statistics -- nn.SyncBatchNorm (their
    defaults), or functools.partial(nn.InstanceNorm2d, affine=True) (model.{idx}.weight / .bias of the norm modules).
    spectral_norm (opt-in, beyond the reference's constructor): every convolution as torch.nn.utils.spectral_norm(conv) leaves it --
    state_dict keys model.{i}.bias, .weight_orig (the parameter), .weight_u, .weight_v (buffers), one power iteration per
    training-mode forward(); the kernels run on W / sigma (spectral_normalize) and the gradient is mapped back to weight_orig
    (spectral_grad_map).  Trainer.batch iterates ONCE per call and uses that one normalised weight for all of the step's D passes.
    final_act (opt-in, beyond the reference's constructor): 'sigmoid' (the reference's nn.Sigmoid) or 'none' -- forward() returns the
    head conv's logits, what Trainer.gan_mode = 'hinge' needs and 'lsgan' / 'vanilla' accept.  nn.Sigmoid has no state: state_dict,
    parameter order and .pth files are the same for both values."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm=False, norm_layer=nn.InstanceNorm2d, spectral_norm=False, final_act='sigmoid'):
        super().__init__()
        if not isinstance(final_act, str) or final_act not in E.DISC_FINAL_ACTS:
            raise ValueError(f"patchgan_amd.Discriminator: final_act must be one of {' | '.join(E.DISC_FINAL_ACTS)}, got {final_act!r}")
        if not isinstance(spectral_norm, bool):
            raise TypeError(f"patchgan_amd.Discriminator: spectral_norm must be a bool, got {spectral_norm!r}")
        kind = E.norm_kind_of(norm_layer, 'patchgan_amd.Discriminator') if norm else 'instance'
        self.engine = E.DiscriminatorEngine(input_nc, ndf, n_layers, norm, norm_kind=kind, spectral=spectral_norm, final_act=final_act)
        self._param_keys = E.param_keys(self.engine.layers)
        self._init_flat(self.engine.layers, self.engine.nparams)

    @property
    def spectral_norm(self):
        return self.engine.spectral

    @property
    def final_act(self):
        """'sigmoid': forward() returns probabilities (the reference); 'none': the head's logits."""
        return self.engine.final_act

    def _spectral_state(self):
        if not self.engine.spectral:
            raise RuntimeError("patchgan_amd.Discriminator was built without spectral_norm=True")
        dev = self.flat.device
        if dev.type != 'cuda':
            raise RuntimeError("patchgan_amd.Discriminator: spectral normalisation runs on a HIP device (discriminator.to('cuda')); "
                               "there is no CPU path")
        if self.sn_eff is None or self.sn_eff.device != dev:
            object.__setattr__(self, 'sn_eff', torch.zeros_like(self.flat))
            # (one workspace for the forward sequence and one for the gradient map: the latter may run on the second stream)
            object.__setattr__(self, 'sn_ws', (E.spectral_workspace(self._layers, dev), E.spectral_workspace(self._layers, dev)))
        return self.sn_eff, self.sn_ws

    def spectral_normalize(self, iterate=None):
        """Normalise now, on the current stream: the persistent effective-weight buffer (the flat buffer's layout and size, a stable
        address) receives W / sigma in every conv weight block and a copy of everything else, and is returned -- what the engine's
        passes take in place of `flat`.  iterate: one power iteration first (u, v updated), None = as torch's hook does, in training
        mode only; without it sigma comes from the stored u, v.  The caller orders this behind an update of the weights in flight
        (Trainer.flush) -- it reads `flat` directly."""
        eff, ws = self._spectral_state()
        E.spectral_fwd(self._layers, self.flat, eff, self.sn_bufs, ws[0], self.training if iterate is None else bool(iterate))
        return eff

    def spectral_grad_map(self, gflat, eff=None, bufs=None):
        """Map the flat gradient `gflat` of a pass that ran on the effective buffer back to the stored weights, in place, on the current
        stream: per layer dW = (dW_hat - <dW_hat, W_hat> u v^T) / sigma with the W_hat, u, v, sigma of the last spectral_normalize()
        (or those given); biases and norm parameters pass through."""
        own, ws = self._spectral_state()
        E.spectral_bwd(self._layers, own if eff is None else eff, self.sn_bufs if bufs is None else bufs, ws[1], gflat)
        return gflat

    def forward(self, input):
        self._pre_access()
        params = [self.get_parameter(k) for k in self._param_keys]
        return _DiscFn.apply(self, input, *params)
