"""UNet generator with the reference's constructor / forward / state_dict surface (patchgan/unet.py:75-134),
executed by hand-written gfx950 kernels (patchgan_amd.engine.GeneratorEngine)."""
import torch
from torch import nn

from . import engine as E
from ._module import FlatParamModule
from .transfer import Transferable


class _UNetFn(torch.autograd.Function):
    """Whole-network autograd node: forward = engine forward, backward = engine backward."""

    @staticmethod
    def forward(ctx, module, x, return_hidden, *params):
        eng = module.engine
        N, C, H, W = x.shape
        dev = module.flat.device
        xin = E.View.alloc(N, H, W, C, dev).from_nchw(x.to(device=dev, dtype=torch.float32))
        gen = E.View.alloc(N, H, W, eng.output_nc, dev)
        seed = module._next_seed() if module.training else 0
        c = eng.forward(module.flat, xin, gen, module.training, seed, bn=module.bn_run())
        module.bn_update(1)          # training mode: this call's batch statistics into the running statistics, as torch does
        ctx.module, ctx.c = module, c
        ctx.need_dx = x.requires_grad
        out = gen.to_nchw()
        if return_hidden:
            hidden = c.hidden.to_nchw()
            ctx.mark_non_differentiable(hidden)   # side output: gradients flow through `out` only
            return out, hidden
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        module, c = ctx.module, ctx.c
        eng = module.engine
        dev = module.flat.device
        g = E.View.alloc(c.N, c.H, c.W, eng.output_nc, dev).from_nchw(gout.to(torch.float32))
        gflat = torch.zeros_like(module.flat)
        dx = eng.backward(module.flat, gflat, c, g, None, need_dx=ctx.need_dx)      # (BatchNorm: with the coefficients saved in c)
        views = E.torch_views(gflat, eng.layers)
        grads = tuple(views[k] for k in module._param_keys)
        return (None, dx.to_nchw() if dx is not None else None, None) + grads


class UNet(FlatParamModule, Transferable):
    """UNet(input_nc, output_nc, nf=64, norm_layer=InstanceNorm2d, use_dropout=False, activation='tanh',
    final_act='softmax') -- reference unet.py:76-78.  norm_layer: nn.InstanceNorm2d, nn.BatchNorm2d or -- for data
    parallelism: the global batch's statistics -- nn.SyncBatchNorm (their defaults), or functools.partial(nn.InstanceNorm2d,
    affine=True): InstanceNorm with a learnable per-channel scale and shift (DownNorm{i} / UpNorm{i} .weight / .bias)."""

    def __init__(self, input_nc, output_nc, nf=64, norm_layer=nn.InstanceNorm2d, use_dropout=False,
                 activation='tanh', final_act='softmax'):
        super().__init__()
        kind = E.norm_kind_of(norm_layer, 'patchgan_amd.UNet')
        self.engine = E.GeneratorEngine(input_nc, output_nc, nf, activation, final_act, use_dropout, norm_kind=kind)
        self._param_keys = E.param_keys(self.engine.layers)
        self._seed_base = int(torch.initial_seed()) & 0xFFFFFFFF
        self._calls = 0
        self._init_flat(self.engine.layers, self.engine.nparams)

    def twin(self, flat):
        """A second UNet with this one's constructor arguments, precision and tuning, in eval mode, whose parameters are views of
        the given flat buffer (this network's packed layout and device) and whose BatchNorm running statistics ARE this network's
        tensors.  Nothing is initialised, so nothing is drawn from torch's RNG (Trainer.ema_generator)."""
        eng = self.engine
        t = UNet.__new__(UNet)
        nn.Module.__init__(t)
        t.engine = E.GeneratorEngine(eng.input_nc, eng.output_nc, eng.nf, eng.activation, eng.final_act, eng.use_dropout,
                                     algo=eng.algo, norm_kind=eng.norm_kind)
        t._param_keys = E.param_keys(t.engine.layers)
        t._seed_base, t._calls = self._seed_base, 0
        t._layers = t.engine.layers
        t.eval()
        t.follow(self, flat)
        return t

    def follow(self, other, flat):
        """Keep a twin() in step with `other`: its device (flat buffer), BatchNorm buffers, precision and tuning."""
        if any(getattr(self, k, None) is not v for k, v in (('flat', flat), ('bn_bufs', other.bn_bufs), ('bn_counters', other.bn_counters))):
            self._bind(flat, other.bn_bufs, other.bn_counters)
        eng, src = self.engine, other.engine
        if (eng.algo, eng.act_bf) != (src.algo, src.act_bf):
            eng.algo, eng.act_bf = src.algo, src.act_bf
            eng._ops, eng._sok = {}, {}
            eng.clear_weight_caches()
        if hasattr(other, 'precision'):
            self.precision = other.precision

    def _next_seed(self):
        self._calls += 1
        return E._mix_seed(self._seed_base, self._calls)

    def forward(self, x, return_hidden=False):
        params = [self.get_parameter(k) for k in self._param_keys]
        return _UNetFn.apply(self, x, return_hidden, *params)
