"""Device engines for the patchGAN hot path: UNet generator and PatchGAN discriminator forward /
backward scheduled as explicit HIP kernel launches through the C ABI (include/patchgan_hip.h).

Data layout in HBM
  * activations: fp32 NHWC.  A `View` is (tensor, element offset, pixel stride ld, N, H, W, C): a channel
    slice of a wider buffer.  Skip connections (reference unet.py:127 ``torch.cat([x, xencs[i]], dim=1)``)
    are never materialised by a copy: decoder level i owns one buffer ``cat_i`` of C_dec + C_skip channels;
    decoder block i-1 writes channels [0, C_dec) and encoder block 6-i writes channels [C_dec, ...) directly.
    The discriminator input cat(x, mask) (trainer.py:65,96,98) is handled the same way.
  * weights: ONE flat fp32 buffer per network holding, per layer, the packed block P[16][a][b] (+ bias).  The
    torch-layout tensor W[a][b][4][4] the reference's state_dict exposes is a *strided view* of that block
    (strides (b, 1, 4ab, ab)), so checkpoints interchange with the reference without any repack kernel, and
    Adam / RCCL all-reduce run over the flat buffer in one launch.

Nothing here touches autograd; `patchgan_amd.unet` / `.disc` wrap the engines in torch.autograd.Function and
`patchgan_amd.trainer` drives them directly.
"""
import ctypes
import os
import functools
import math
import threading

import numpy as np

import torch
from torch import nn

from . import _lib as L

_MASK64 = (1 << 64) - 1
# PATCHGAN_ALGO=direct forces the one-thread-per-output kernels everywhere (debugging aid); =bf16 selects the bf16
# MFMA variants (fp32 tensors, bf16 multiply, fp32 accumulate); default = the fp32 MFMA path
DEFAULT_ALGO = {'direct': L.ALGO_DIRECT, 'mfma': L.ALGO_MFMA, 'bf16': L.ALGO_BF16}.get(__import__('os').environ.get('PATCHGAN_ALGO', ''), L.ALGO_AUTO)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    # the raw handle of torch's current stream on the current device, without building a torch.cuda.Stream object per launch
    # (torch.cuda.current_stream() was a quarter of the step's host time: 170 calls per step, tools/host_profile.py)
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class View:
    """NHWC channel-slice of a device buffer; `bf` = the buffer holds bf16 elements (bf16 activation storage), else fp32.
    `off` and `ld` count elements of the buffer's own type."""
    __slots__ = ('t', 'off', 'ld', 'N', 'H', 'W', 'C', 'bf')

    def __init__(self, t, off, ld, N, H, W, C, bf=False):
        self.t, self.off, self.ld, self.N, self.H, self.W, self.C, self.bf = t, off, ld, N, H, W, C, bf

    @staticmethod
    def alloc(N, H, W, C, device, zero=False, bf=False):
        t = (torch.zeros if zero else torch.empty)(N * H * W * C, dtype=torch.bfloat16 if bf else torch.float32, device=device)
        return View(t, 0, C, N, H, W, C, bf)

    def ptr(self):
        return self.t.data_ptr() + self.off * (2 if self.bf else 4)

    def padded8(self):
        """This fp32 view (C <= 8) as a bf16 tensor in 8-channel pixels (ld 8, pad channels zero): the layout in which the bf16
        kernels take the image-facing tensors (pg_pad8_bf16)."""
        assert not self.bf and self.C <= 8
        t = torch.empty(self.npix * 8, dtype=torch.bfloat16, device=self.t.device)
        L.check(L.load().pg_pad8_bf16(self.ptr(), self.ld, t.data_ptr(), self.npix, self.C, _stream()), 'pg_pad8_bf16')
        return View(t, 0, 8, self.N, self.H, self.W, self.C, True)

    def channels(self, c0, c):
        assert 0 <= c0 and c0 + c <= self.C
        return View(self.t, self.off + c0, self.ld, self.N, self.H, self.W, c, self.bf)

    def samples(self, n0, n):
        assert 0 <= n0 and n0 + n <= self.N
        return View(self.t, self.off + n0 * self.H * self.W * self.ld, self.ld, n, self.H, self.W, self.C, self.bf)

    def converted(self, bf):
        """A dense copy of this view in the other storage type (pg_act_fwd_t with PG_ACT_NONE), or self if it already has it."""
        if self.bf == bf:
            return self
        out = View.alloc(self.N, self.H, self.W, self.C, self.t.device, bf=bf)
        L.check(L.load().pg_act_fwd_t(self.ptr(), self.ld, out.ptr(), out.ld, self.npix, self.C, L.ACT_NONE, 0.0, 0, _stream(),
                                      (1 if self.bf else 0) | (2 if bf else 0)), 'pg_act_fwd_t')
        return out

    @property
    def HW(self):
        return self.H * self.W

    @property
    def extent_bytes(self):
        """Bytes from this view's first element to the end of its last pixel row (what a kernel's 32-bit offsets must span)."""
        return self.npix * self.ld * (2 if self.bf else 4)

    @property
    def npix(self):
        return self.N * self.H * self.W

    def to_nchw(self):
        """Materialise as a contiguous NCHW fp32 torch tensor (API edge)."""
        if self.bf:
            return self.converted(False).to_nchw()
        out = torch.empty(self.N, self.C, self.H, self.W, dtype=torch.float32, device=self.t.device)
        L.check(L.load().pg_nhwc_to_nchw(self.ptr(), self.ld, out.data_ptr(), self.N, self.C, self.H, self.W,
                                         _stream()), 'pg_nhwc_to_nchw')
        return out

    def from_nchw(self, src):
        """Fill from a contiguous NCHW torch tensor of shape [N, C, H, W]."""
        assert tuple(src.shape) == (self.N, self.C, self.H, self.W), (tuple(src.shape), (self.N, self.C, self.H, self.W))
        assert not self.bf, 'API-edge layout kernels write fp32 views'
        src = src.contiguous()
        L.check(L.load().pg_nchw_to_nhwc(src.data_ptr(), self.ptr(), self.ld, self.N, self.C, self.H, self.W,
                                         _stream()), 'pg_nchw_to_nhwc')
        return self

    def from_u8(self, src, div=255.0):
        """Fill from decoded image bytes: uint8 device tensor [N, H, W, C] -> value / div (reference io.py:42)."""
        assert src.dtype == torch.uint8 and tuple(src.shape) == (self.N, self.H, self.W, self.C), tuple(src.shape)
        src = src.contiguous()
        L.check(L.load().pg_u8_to_f32(src.data_ptr(), self.ptr(), self.ld, self.npix, self.C, div, _stream()), 'pg_u8_to_f32')
        return self

    def from_labels(self, src, labels, add=1):
        """Fill with the one-hot mask of a uint8 label map [N, H, W]: channel i = ((uint8)(src + add) == labels[i])
        (reference io.py:43,53-56)."""
        assert src.dtype == torch.uint8 and tuple(src.shape) == (self.N, self.H, self.W), tuple(src.shape)
        assert len(labels) == self.C, (len(labels), self.C)
        src = src.contiguous()
        arr = (ctypes.c_int * len(labels))(*[int(v) for v in labels])
        L.check(L.load().pg_labels_to_onehot(src.data_ptr(), self.ptr(), self.ld, self.npix, arr, len(labels), add, _stream()),
                'pg_labels_to_onehot')
        return self


def din_fill(x, y, real, fake):
    """real = x | y, fake = x | 0 (NHWC fp32 views of one pixel stride, x / y contiguous NCHW): the discriminator's concatenated inputs
    (trainer.py:65,96,98) in one launch; the generator's head writes its output into fake's mask channels later in the step."""
    N, Cx, H, W = x.shape
    Cy = y.shape[1]
    assert tuple(y.shape) == (N, Cy, H, W) and (real.N, real.H, real.W, real.C) == (N, H, W, Cx + Cy) == (fake.N, fake.H, fake.W, fake.C)
    assert real.ld == fake.ld and not real.bf and not fake.bf
    x, y = x.contiguous(), y.contiguous()
    L.check(L.load().pg_din_fill(x.data_ptr(), y.data_ptr(), real.ptr(), fake.ptr(), real.ld, N, Cx, Cy, H, W, _stream()), 'pg_din_fill')


# ------------------------------------------------------------------------------------------------
# execution state: workspaces (split-K slabs) and the second stream, owned by whoever drives the engines
# ------------------------------------------------------------------------------------------------
# Weight gradients on a second stream.  Inside a network's backward pass a layer's weight gradient and its data gradient both start
# from dy and are independent of each other; enqueued on one stream their kernels run strictly one after the other, and every kernel
# whose grid is one round of workgroups loses its ramp, its lock-step prologue / epilogue phases and its tail (EXPERIMENTS.md, "the fp32
# polyphase GEMM's tile life": ~15-20 % of such a launch).  With the weight-gradient chain on a second stream (its own workspace) the
# two chains' kernels fill each other's gaps: cfg2 fp32 8.85 -> 8.68 ms per step with only the encoder's and the discriminator's
# weight gradients moved.  Same kernels, same order of every floating-point sum: bit-identical results.  The operands are referenced
# until the streams join at the end of the backward pass (the caching allocator must not hand them out meanwhile).  Off under the
# launch profiler, for bf16 networks' weight gradients and inside a hipGraph capture; it costs ~0.6 ms of host time per step (26 stream
# hand-overs), so it pays where the device step is several times the host's enqueue time (the Trainer measures both and picks: cfg2
# fp32 8.95 -> 8.65 ms, cfg4 fp32 16.7 -> 16.5; cfg1's 2.9-ms step stays on the captured graph).


class Exec:
    """Execution state of ONE driver of the engines (a Trainer; or a device's default for stand-alone module calls): the split-K
    workspace per stream and the book-keeping of a two-stream step.  Nothing in here is shared between owners -- two Trainers (also on
    different GPUs, also on different threads) never see each other's flags, held operands or buffers, and everything is released with
    the owner (or by release()).  The second STREAM is the device's (one per device, _SECOND_STREAMS): owners on one device use it in
    order, each behind its own hand-overs.

      enabled   set by the owner per step: this step may use the second stream
      allow     inside a backward pass: weight gradients go to the second stream
      inside    what is enqueued right now goes to the second stream (its own workspace)
      pending   something was enqueued under on_side() and has not been joined
      keep      operands of second-stream launches, referenced until the join
      ws_gen    counts workspace (re)allocations: a captured graph holds the buffers it was captured with (Trainer._capture)"""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else None
        self.enabled = self.allow = self.inside = self.pending = False
        self.stream = None
        self.keep = []
        self.keep_ptrs = set()
        self.keep_bytes = 0
        self.ws = {}
        self.ws_gen = 0
        self._prev = []

    def side_stream(self):
        """The second stream of a two-stream step, created on first use ON THE OWNER'S DEVICE."""
        if self.stream is None:
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            st = _SECOND_STREAMS.get(dev.index)
            if st is None:
                st = _SECOND_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
            self.stream = st
        return self.stream

    def workspace(self, nbytes, device):
        if self.device is not None and device != self.device:
            raise RuntimeError(f'patchgan_amd: engine call on {device} under an execution state bound to {self.device}')
        ws = self.ws.get(self.inside)
        if ws is None or ws.numel() < nbytes:
            ws = self.ws[self.inside] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self.ws_gen += 1
        return ws

    def buffers(self):
        """The device buffers launches under this state write into besides their arguments (what a captured graph must keep alive)."""
        return list(self.ws.values())

    def release(self):
        """Give the workspaces back to the allocator (the second stream is joined first)."""
        if self.stream is not None and (self.keep or self.pending):
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self.keep.clear()
        self.keep_ptrs.clear()
        self.keep_bytes = 0
        self.pending = self.allow = self.inside = False
        self.ws.clear()
        self.ws_gen += 1

    def __enter__(self):
        self._prev.append(getattr(_TLS, 'cur', None))          # (a stack: flush() inside batch() enters the same state again)
        _TLS.cur = self
        return self

    def __exit__(self, *exc):
        _TLS.cur = self._prev.pop()
        return False


_TLS = threading.local()
# ONE second stream per device for every owner on it.  A stream is a device resource: torch hands out streams from a fixed pool and the HIP
# runtime maps each onto one of its hardware queues -- a process that went through several trainers (bench.py's legs) otherwise ended up
# with a second stream sharing the compute stream's hardware queue: the fourth trainer's two-stream step took 6.9 ms instead of 2.5.
# In-order sharing is harmless: every hand-over to / from it is a stream wait, and owners' flags, held operands and workspaces stay
# their own.
_SECOND_STREAMS = {}
_DEFAULT_EXEC = {}       # device index -> Exec of stand-alone module calls (UNet(...)(x), predict_image): one workspace, never a second stream


def cur_exec(device=None):
    """The execution state of the running driver (`with exec:`), or the device's default one for stand-alone module calls."""
    ex = getattr(_TLS, 'cur', None)
    if ex is not None:
        return ex
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    ex = _DEFAULT_EXEC.get(device.index)
    if ex is None:
        ex = _DEFAULT_EXEC[device.index] = Exec(device)
    return ex


def release_workspaces():
    """Free the default execution states' workspaces (stand-alone module calls; a Trainer's go with the Trainer or by
    Trainer.release())."""
    for ex in _DEFAULT_EXEC.values():
        ex.release()
    _DEFAULT_EXEC.clear()


# the owner joins every KEEP_LIMIT_BYTES of operands held for the second stream (with defer_join nearly all backward
# temporaries of a pass were live at once; joining costs one stream wait, ~10 us)
KEEP_LIMIT_BYTES = 3 << 30


class on_side:
    """`with on_side():` -- what is enqueued inside goes to the second stream (after everything enqueued so far), with that stream's
    own workspace; the caller joins with side_join() before it reads the results on its own stream.  Tensors allocated inside belong
    to the second stream's allocator pool: safe as long as every later use on the second stream is again behind such a hand-over
    (it is: each one starts with wait_stream)."""
    def __enter__(self):
        ex = self._ex = cur_exec()
        side = ex.side_stream()
        side.wait_stream(torch.cuda.current_stream())
        self._ctx = torch.cuda.stream(side)
        self._ctx.__enter__()
        self._was = ex.inside
        ex.inside = ex.pending = True
        return side

    def __exit__(self, *exc):
        self._ex.inside = self._was
        return self._ctx.__exit__(*exc)


def _side_begin(allow):
    # (not inside a hipGraph capture: a captured two-branch step replays SLOWER than the one-stream one, 9.03 vs 8.96 ms at cfg2)
    ex = cur_exec()
    # (nor inside on_side(): a pass the caller has put on the second stream as a whole runs its chains one after the other there)
    ex.allow = (bool(allow) and ex.enabled and not ex.inside and WGRAD_SIDE and PROFILER is None
                and not torch.cuda.is_current_stream_capturing())


def side_join():
    """The caller's join: of a backward pass called with defer_join=True and of anything enqueued under on_side() (no-op if nothing
    is pending)."""
    _side_join(True)


def _side_join(explicit=False):
    """The weight gradients enqueued on the second stream are complete for the current stream; their operands may be freed.  (The
    join at the end of a backward pass does not wait for work the CALLER put on the second stream under on_side(): only the caller's
    own side_join() does.)"""
    ex = cur_exec()
    ex.allow = False
    if ex.keep or (explicit and ex.pending):
        torch.cuda.current_stream().wait_stream(ex.stream)
        ex.keep.clear()
        ex.keep_ptrs.clear()
        ex.keep_bytes = 0
        ex.pending = False


def side_producers():
    """Streams besides the current one that may still be writing weight gradients (data parallelism: the bucket all-reduce waits
    for them too, parallel.Dist.all_reduce_side)."""
    ex = cur_exec()
    return [ex.stream] if (ex.stream is not None and (ex.keep or ex.pending)) else []


def _workspace(nbytes, device):
    return cur_exec(device).workspace(nbytes, device)


class LaunchProfiler:
    """Optional per-launch timing of the conv kernels with HIP events on the launch stream (bench.py's roofline
    leg).  Enabled by assigning an instance to ``engine.PROFILER``; costs two event records per launch."""
    def __init__(self, only=None):
        self.records = []   # (symbol, split, flops, start_event, end_event)
        self.only = only    # symbol: time only this kernel's launches
        self.limit = None   # stop arming events after this many records (bench.py: a bounded sample of the timed region)
        self._pool = []

    def reserve(self, n):
        """Create n events ahead of the timed region: creating (and first-recording, which is what makes torch allocate the
        hipEvent_t) an event per launch inside it costs host time and a stream operation each."""
        for _ in range(n):
            self._pool.append(self._new_event())

    def _new_event(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()          # torch creates the hipEvent_t lazily, at the first record: force it (the C side re-records the event)
        return e

    def launch(self, op, opcode, fn, io=0):
        if op.algo & L.ALGO_MASK == L.ALGO_DIRECT:
            return fn()
        sym, split = op.describe(opcode, io)
        if (self.only is not None and sym != self.only) or (self.limit is not None and len(self.records) >= self.limit):
            return fn()
        e0, e1 = self._event(), self._event()
        # the C ABI records the pair tightly around the main GEMM kernel of this call (not its split-K reduce)
        L.check(L.load().pg_conv_time_next(e0.cuda_event, e1.cuda_event), 'pg_conv_time_next')
        fn()
        self.records.append((sym, split, op.flops, op.kernel_flops(opcode, io), op.useful_flops(opcode, io), e0, e1))

    def launch2(self, op, opcodes, fn, io=0):
        """A fused call with two main GEMM kernels (pg_conv4x4_bwd_big): one event pair per kernel."""
        if op.algo & L.ALGO_MASK == L.ALGO_DIRECT:
            return fn()
        syms = [op.describe(oc, io)[0] for oc in opcodes]
        if (self.only is not None and self.only not in syms) or (self.limit is not None and len(self.records) >= self.limit):
            return fn()
        ev = [self._event() for _ in range(4)]
        L.check(L.load().pg_conv_time_next2(*[e.cuda_event for e in ev]), 'pg_conv_time_next2')
        fn()
        for i, oc in enumerate(opcodes):
            if self.only is None or syms[i] == self.only:
                self.records.append((syms[i], op.describe(oc, io)[1], op.flops, op.kernel_flops(oc, io), op.useful_flops(oc, io), ev[2 * i], ev[2 * i + 1]))

    def _event(self):
        if self._pool:
            return self._pool.pop()
        return self._new_event()

    def summary(self):
        """{symbol: dict(launches, ms, flops, kflops, uflops)} over every launch of that kernel symbol (all split-K factors, like a
        rocprofv3 --stats row): flops = algorithmic (direct-convolution) FLOPs of the layers, kflops = FLOPs the kernel
        executed (fewer for Winograd kernels; ragged edge tiles count as whole tiles), uflops = the kernel's algorithm on the exact
        extents (no tile padding) -- call after a device synchronize."""
        out = {}
        for sym, split, flops, kflops, uflops, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            d = out.setdefault(sym, dict(launches=0, ms=0.0, flops=0.0, kflops=0.0, uflops=0.0))
            d['launches'] += 1
            d['ms'] += ms
            d['flops'] += flops
            d['kflops'] += kflops
            d['uflops'] += uflops
        return out


PROFILER = None
_MAX_TENSOR_BYTES = None      # pg_conv_max_tensor_bytes(), read once


class ConvOp:
    """One 4x4 / padding-1 convolution layer bound to its geometry: the three kernels that touch its weights."""

    def __init__(self, N, Hb, Wb, Ca, Cb, stride, algo=L.ALGO_AUTO):
        Hs = (Hb - 2) // stride + 1
        Ws = (Wb - 2) // stride + 1
        if Hb < 2 or Wb < 2 or Hs < 1 or Ws < 1:
            raise RuntimeError(f"Kernel size can't be greater than actual input size ({Hb}x{Wb}, 4x4 kernel, pad 1)")
        self.g = L.ConvGeom(N, Hb, Wb, Hs, Ws, Ca, Cb, stride)
        self.N, self.Hb, self.Wb, self.Hs, self.Ws, self.Ca, self.Cb, self.stride = N, Hb, Wb, Hs, Ws, Ca, Cb, stride
        self.algo = algo
        lib = L.load()
        self.ws_bytes = max(int(lib.pg_conv_workspace_bytes(ctypes.byref(self.g), op)) for op in (0, 1, 2, 3))
        self._desc = {}

    @property
    def ws_arg(self):
        """The workspace size every query (pg_conv_kernel, pg_conv_u_bytes, pg_conv_stats_chunks, ...) AND every launch of this
        op passes to the C ABI: the SAME number on both sides, so a hand-over sized by a query can never meet a launch that
        planned with a different workspace (the device buffer itself is shared and may be larger)."""
        return max(self.ws_bytes, 1 << 20)

    def _ws(self, device):
        ws = _workspace(self.ws_bytes, device)          # (at least ws_arg bytes: _workspace never allocates less than 1 MiB)
        return ws.data_ptr(), self.ws_arg

    @property
    def flops(self):
        """Algorithmic FLOPs of any of the three kernels on this geometry: 2 * N*Hs*Ws * 16 * Ca * Cb."""
        return 2.0 * self.N * self.Hs * self.Ws * 16 * self.Ca * self.Cb

    def kernel_flops(self, opcode, io=0):
        """FLOPs the main GEMM kernel of this call really executes on the MFMA pipe: the algorithmic count for the implicit
        GEMM kernels, 2.25-4x fewer for the Winograd kernels (their tile counts include the ragged-edge padding)."""
        return self._describe(opcode, io)[2]

    def useful_flops(self, opcode, io=0):
        """The main GEMM kernel's FLOPs without the padding of ragged edge tiles to whole tiles (pg_conv_kernel_flops): equal to
        kernel_flops for the implicit-GEMM kernels, 6-27 % below it for the Winograd kernels at cfg2."""
        ex, us = ctypes.c_double(0), ctypes.c_double(0)
        L.check(L.load().pg_conv_kernel_flops(ctypes.byref(self.g), opcode + 16 * (self.algo | io), self.ws_arg, ctypes.byref(ex),
                                              ctypes.byref(us)), 'pg_conv_kernel_flops')
        return us.value

    def describe(self, opcode, io=0):
        """(kernel symbol, split-K factor) of the main GEMM kernel the C ABI launches for this op (pg_conv_kernel: the
        dispatch code itself reports it).  io: the PG_IO_* bits of the call (bf16 activation storage)."""
        return self._describe(opcode, io)[:2]

    def _describe(self, opcode, io=0):
        key = (opcode, io)
        if key not in self._desc:
            name = ctypes.create_string_buffer(128)
            s, fl = ctypes.c_int(0), ctypes.c_double(0)
            L.check(L.load().pg_conv_kernel(ctypes.byref(self.g), opcode + 16 * (self.algo | io), self.ws_arg, name, 128,
                                            ctypes.byref(s), ctypes.byref(fl)), 'pg_conv_kernel')
            self._desc[key] = (name.value.decode(), s.value, fl.value)
        return self._desc[key]

    @staticmethod
    def _aligned(*views):
        return all(v.ld % 4 == 0 and v.ptr() % 16 == 0 and not v.bf for v in views)     # (the Winograd hand-overs are fp32 paths)

    @staticmethod
    def fits(*views):
        """Every view is addressable by the buffer-load kernels (pg_conv_max_tensor_bytes: 32-bit byte offsets).  The C side's size
        queries see the geometry only; the launches also see the views and leave the fast / bf16 paths for a tensor beyond this
        limit -- so hand-overs (part, v_keep, u_cache, mul_t) are planned only for views that fit."""
        global _MAX_TENSOR_BYTES
        if _MAX_TENSOR_BYTES is None:
            _MAX_TENSOR_BYTES = int(L.load().pg_conv_max_tensor_bytes())
        return all(v.extent_bytes < _MAX_TENSOR_BYTES for v in views)

    @staticmethod
    def _io(big, small):
        return (L.IO_BIG_BF16 if big.bf else 0) | (L.IO_SMALL_BF16 if small.bf else 0)

    def _query(self, key, fn):
        if key not in self._desc:
            self._desc[key] = int(fn())
        return self._desc[key]

    def stats_chunks(self, opcode, view_in, view_out):
        """Partial-sum chunks per sample the kernel of big2small (0) / small2big (1) can emit next to its output (K5: InstanceNorm
        statistics from the conv epilogue); 0 = not on this path (or the views are not 16-byte aligned)."""
        big, small = (view_in, view_out) if opcode == 0 else (view_out, view_in)
        io = self._io(big, small)
        if not self.fits(view_in, view_out):
            return 0
        if io:      # bf16 tensors: the LDS-DMA kernels' STATS epilogue (both tensors bf16, 16-byte-aligned views)
            if io != L.IO_MASK or not all(v.ptr() % 16 == 0 and v.ld % 8 == 0 for v in (view_in, view_out)):
                return 0
        elif not self._aligned(view_out) or (not self._aligned(view_in) and not (opcode == 0 and self.Cb <= 3)):
            return 0          # (the image-facing kernel k_b2s_tapkp gathers <= 3-channel pixels by scalars: any input view)
        return self._query(('chunks', opcode, io), lambda: L.load().pg_conv_stats_chunks(ctypes.byref(self.g), opcode, self.algo | io,
                                                                                        self.ws_arg))

    def u_bytes(self, opcode, io=0):
        """Bytes of the transformed weights the kernel of big2small (0) / small2big (1) works from (0: no weight transform on
        this path): what a caller-owned cache for pg_conv_extras.u_cache must hold.  io: the PG_IO_* bits of the call (the bf16
        kernels on bf16 tensors work from a packed bf16 copy of the weights)."""
        return self._query(('u', opcode, io), lambda: L.load().pg_conv_u_bytes(ctypes.byref(self.g), opcode, self.algo | io,
                                                                               self.ws_arg))

    def v_bytes(self):
        """Bytes of the polyphase-transformed `big` tensor that big2small can keep (v_keep) for the weight gradient of the
        same layer (v_pre); 0 when the two calls do not both take the polyphase Winograd path."""
        return self._query(('v',), lambda: L.load().pg_conv_v_bytes(ctypes.byref(self.g), self.algo, self.ws_arg))

    def keep_v(self, want, *views):
        """The buffer in which big2small keeps its transformed `big` tensor for the weight gradient of the same layer (v_keep, then
        v_pre), or None: nobody wants it (`want`, KEEP_V), the two calls do not both take the polyphase Winograd path on this geometry
        (v_bytes) or the views the calls will see are not ones that path takes."""
        vb = self.v_bytes() if (want and KEEP_V and self._aligned(*views) and self.fits(*views)) else 0
        return torch.empty(vb, dtype=torch.uint8, device=views[0].t.device) if vb else None

    def halves_same(self, whole):
        """big2small of this op (N samples) and of `whole` (the same layer on 2 N samples) do the same arithmetic per sample
        (pg_conv_batch_halves_same: same kernel, no split over K, V kept in both or in neither): two calls of this op on the halves
        of a 2 N batch fill what one call of `whole` fills, bit for bit."""
        assert whole.g.key()[1:] == self.g.key()[1:] and whole.N == 2 * self.N and whole.algo == self.algo
        return bool(self._query(('halves', whole.ws_arg), lambda: L.load().pg_conv_batch_halves_same(
            ctypes.byref(self.g), self.algo, self.ws_arg, whole.ws_arg)))

    def v_part(self, whole, n0):
        """(v_stride, v_tile0) with which big2small of this op, run on samples [n0, n0 + N) of the batch of `whole`, keeps its
        transformed input in the buffer of whole.v_bytes() bytes: V[point][tile][k], the tiles of the whole batch inside every
        point's plane."""
        points, k = (16, 4 * self.Cb) if self.stride == 2 else (36, self.Cb)
        stride = whole.v_bytes() // (4 * points)
        return stride, n0 * (stride // k) // whole.N

    @staticmethod
    def _extras(part=None, v_keep=None, v_pre=None, u_cache=None, u_valid=False, mul=None, v_part=(0, 0)):
        if part is None and v_keep is None and v_pre is None and u_cache is None and mul is None:
            return None
        p = lambda t: t.data_ptr() if t is not None else None
        mt, ml, ma = (mul[0].ptr(), mul[0].ld, mul[1]) if mul is not None else (None, 0, 0)
        return L.ConvExtras(p(part), p(v_keep), p(v_pre), p(u_cache), 1 if u_valid else 0, mt, ml, ma, v_part[0], v_part[1])

    def mul_ok(self, small, big, t):
        """small2big(small -> big) can fold `big *= f'(t)` into its epilogue (pg_conv_extras.mul_t): the kernel of this call supports
        it and the tensors satisfy its alignment; t must have big's shape and storage type."""
        if t.bf != big.bf or (t.N, t.H, t.W, t.C) != (big.N, big.H, big.W, big.C) or not self.fits(small, big, t):
            return False
        need = (big, t) if self.Ca == 1 else (small, big, t)       # (the one-channel kernel reads `small` by scalars)
        if not all(v.ptr() % 16 == 0 and v.ld % (8 if v.bf else 4) == 0 for v in need):
            return False
        io = self._io(big, small)
        return bool(self._query(('mul', io), lambda: L.load().pg_conv_mul_ok(ctypes.byref(self.g), self.algo | io,
                                                                              self.ws_arg)))

    def big2small(self, big, P, p_off, bias, b_off, small, act=L.ACT_NONE, part=None, v_keep=None, u_cache=None, u_valid=False,
                  v_part=(0, 0)):
        """part / v_keep / u_cache: the optional hand-overs of pg_conv_extras (sizes: stats_chunks(0), v_bytes(), u_bytes(0)).
        v_part: v_keep is the buffer of this layer on a larger batch and this call fills its own rows of it (see v_part())."""
        assert (big.N, big.H, big.W, big.C) == (self.N, self.Hb, self.Wb, self.Cb), 'big view mismatch'
        assert (small.N, small.H, small.W, small.C) == (self.N, self.Hs, self.Ws, self.Ca), 'small view mismatch'
        wp, wn = self._ws(P.device)
        args = (big.ptr(), big.ld, L.ptr(P, p_off), L.ptr(bias, b_off) if bias is not None else None, small.ptr(), small.ld,
                ctypes.byref(self.g), act, self.algo | self._io(big, small), wp, wn, _stream())
        x = self._extras(part=part, v_keep=v_keep, u_cache=u_cache, u_valid=u_valid, v_part=v_part if v_keep is not None else (0, 0))

        def go():
            if x is None:
                L.check(L.load().pg_conv4x4_big2small(*args), 'pg_conv4x4_big2small')
            else:
                L.check(L.load().pg_conv4x4_big2small_x(*args, ctypes.byref(x)), 'pg_conv4x4_big2small_x')
        PROFILER.launch(self, 0, go, self._io(big, small)) if PROFILER is not None else go()

    def small2big(self, small, P, p_off, bias, b_off, big, act=L.ACT_NONE, part=None, u_cache=None, u_valid=False, mul=None):
        """mul = (t, act code): big = conv(...) * f'(t), the activation backward of the layer below folded into the epilogue
        (only where mul_ok(small, big, t))."""
        assert (big.N, big.H, big.W, big.C) == (self.N, self.Hb, self.Wb, self.Cb), 'big view mismatch'
        assert (small.N, small.H, small.W, small.C) == (self.N, self.Hs, self.Ws, self.Ca), 'small view mismatch'
        wp, wn = self._ws(P.device)
        args = (small.ptr(), small.ld, L.ptr(P, p_off), L.ptr(bias, b_off) if bias is not None else None, big.ptr(), big.ld,
                ctypes.byref(self.g), act, self.algo | self._io(big, small), wp, wn, _stream())
        x = self._extras(part=part, u_cache=u_cache, u_valid=u_valid, mul=mul)

        def go():
            if x is None:
                L.check(L.load().pg_conv4x4_small2big(*args), 'pg_conv4x4_small2big')
            else:
                L.check(L.load().pg_conv4x4_small2big_x(*args, ctypes.byref(x)), 'pg_conv4x4_small2big_x')
        PROFILER.launch(self, 1, go, self._io(big, small)) if PROFILER is not None else go()

    def wgrad(self, small, big, dP, p_off, dbias=None, b_off=0, v_pre=None):
        """v_pre: the transformed `big` tensor kept by this layer's big2small(..., v_keep=) (same tensor, v_bytes() > 0)."""
        assert (big.N, big.H, big.W, big.C) == (self.N, self.Hb, self.Wb, self.Cb), 'big view mismatch'
        assert (small.N, small.H, small.W, small.C) == (self.N, self.Hs, self.Ws, self.Ca), 'small view mismatch'
        wp, wn = self._ws(dP.device)
        args = (small.ptr(), small.ld, big.ptr(), big.ld, L.ptr(dP, p_off), L.ptr(dbias, b_off) if dbias is not None else None,
                ctypes.byref(self.g), self.algo | self._io(big, small), wp, wn, _stream())
        x = self._extras(v_pre=v_pre)

        def go():
            if x is None:
                L.check(L.load().pg_conv4x4_wgrad(*args), 'pg_conv4x4_wgrad')
            else:
                L.check(L.load().pg_conv4x4_wgrad_x(*args, ctypes.byref(x)), 'pg_conv4x4_wgrad_x')
        ex = cur_exec(dP.device)
        if ex.allow:
            # on the second stream (see Exec): after everything enqueued so far (dy is ready), with that stream's own workspace
            side = ex.side_stream()
            side.wait_stream(torch.cuda.current_stream())
            ex.keep.append((small.t, big.t, v_pre, dP))
            # what this call adds to the bytes held alive: each backing storage once (the skip buffers are shared by several
            # layers' views), plus the transformed input handed over from the forward pass
            for t in (small.t, big.t, v_pre):
                if t is not None and t.data_ptr() not in ex.keep_ptrs:
                    ex.keep_ptrs.add(t.data_ptr())
                    ex.keep_bytes += t.numel() * t.element_size()
            was, ex.inside = ex.inside, True
            try:
                with torch.cuda.stream(side):
                    wp2, wn2 = self._ws(dP.device)
                    args = args[:8] + (wp2, wn2, _stream())
                    go()
            finally:
                ex.inside = was
            if ex.keep_bytes > KEEP_LIMIT_BYTES:
                # bound what the second stream keeps alive: an intermediate join (the chains re-synchronise once; same results)
                torch.cuda.current_stream().wait_stream(side)
                ex.keep.clear()
                ex.keep_ptrs.clear()
                ex.keep_bytes = 0
            return
        PROFILER.launch(self, 2, go, self._io(big, small)) if PROFILER is not None else go()

    def bwd_big(self, small, big, P, dP, p_off, dsmall, u_cache=None, u_valid=False):
        """Weight gradient (small = x, big = dy) and data gradient (big -> small) of a ConvTranspose2d layer in one call; where
        both run the polyphase Winograd path the transformed dy is computed once and shared (pg_conv4x4_bwd_big).
        u_cache / u_valid: the data gradient's transformed weights, as for big2small."""
        assert (big.N, big.H, big.W, big.C) == (self.N, self.Hb, self.Wb, self.Cb), 'big view mismatch'
        assert (small.N, small.H, small.W, small.C) == (self.N, self.Hs, self.Ws, self.Ca), 'small view mismatch'
        assert (dsmall.N, dsmall.H, dsmall.W, dsmall.C) == (self.N, self.Hs, self.Ws, self.Ca), 'dsmall view mismatch'
        wp, wn = self._ws(P.device)

        def go():
            assert small.bf == big.bf == dsmall.bf, 'bwd_big: one storage type for the three activation tensors'
            args = (small.ptr(), small.ld, big.ptr(), big.ld, L.ptr(P, p_off), L.ptr(dP, p_off), dsmall.ptr(), dsmall.ld,
                    ctypes.byref(self.g), self.algo | self._io(big, small), wp, wn, _stream())
            if u_cache is None:
                L.check(L.load().pg_conv4x4_bwd_big(*args), 'pg_conv4x4_bwd_big')
            else:
                x = self._extras(u_cache=u_cache, u_valid=u_valid)
                L.check(L.load().pg_conv4x4_bwd_big_x(*args, ctypes.byref(x)), 'pg_conv4x4_bwd_big_x')
        PROFILER.launch2(self, (2, 0), go, self._io(big, small)) if PROFILER is not None else go()


def _bf16_tensors_ok(ops, ld_mult=1):
    """Every one of these layers has bf16-tensor kernels for its three ops at this geometry (pg_conv_kernel names them): otherwise
    the caller keeps fp32 activation storage for this extent (e.g. 7 x 7 maps on channel counts the LDS-DMA weight gradient does
    not take: the register-staged kernel's pixel decode needs power-of-two or >= 16-wide maps).  And every tensor those kernels
    would see stays below pg_conv_max_tensor_bytes (bf16 tensors have no kernel beyond it; fp32 ones fall back to the generic
    kernels): ld_mult = the widest buffer an interior tensor is a channel slice of, in multiples of its own channel count (2 for
    the generator's skip-connection buffers)."""
    if _MAX_TENSOR_BYTES is None:
        ConvOp.fits()
    for op in ops:
        if max(op.N * op.Hb * op.Wb * op.Cb, op.N * op.Hs * op.Ws * op.Ca) * ld_mult * 2 >= _MAX_TENSOR_BYTES:
            return False
    return all('bf16' in op.describe(oc, L.IO_MASK)[0] for op in ops for oc in (0, 1, 2))


class UCache(dict):
    """A network's transformed / packed weights for ONE weight version: key -> device buffer (see _ucache).  `log` records how each
    entry was made -- (key, op, opcode, io, p_off, bytes) -- so that the engine can fill the same set in one launch next time."""

    def __init__(self, pool=None):
        super().__init__()
        self.log = []
        self.pool = pool if pool is not None else {}      # key -> device buffer, reused from step to step (see _WeightPrep)

    def buffer(self, key, nb, dev):
        """The device buffer of entry `key`: the pool's (same stream as every reader and writer of it, so reusing it for the next
        weight version needs no synchronisation), allocated on first use -- no allocator traffic per step."""
        buf = self.pool.get(key)
        if buf is None or buf.numel() != nb or buf.device != dev:
            buf = self.pool[key] = torch.empty(nb, dtype=torch.uint8, device=dev)
        return buf


def _ucache(ucache, li, opcode, op, dev, src, dst, p_off=None):
    """(buffer, valid) of the transformed / packed weights of layer li / direction opcode in the caller's per-step cache (a dict that
    lives exactly as long as the weights stay unchanged).  On bf16 tensors one packed bf16 copy serves both directions of a layer (the
    small -> big kernel stages it transposed), so the two directions share an entry."""
    if ucache is None or not CACHE_U or not ConvOp.fits(src, dst):
        return None, False
    big, small = (src, dst) if opcode == 0 else (dst, src)
    io = ConvOp._io(big, small)
    if io:      # bf16 tensors: the LDS-DMA kernels' packed bf16 weights (16-byte-aligned views)
        if not all(v.ptr() % 16 == 0 and v.ld % (8 if v.bf else 4) == 0 for v in (src, dst)):
            return None, False
    elif not ConvOp._aligned(src, dst):
        return None, False
    nb = op.u_bytes(opcode, io)
    if not nb:
        return None, False
    # (the window-staged kernel k_conv_bf16r reads weight fragments straight from global memory and takes a fragment-ordered pack of its
    #  own per direction: its layers keep one entry per direction)
    shared = (io == L.IO_MASK and op.Cb > 8 and not (op.algo & L.TUNE_BF16X_RING)
              and not op.describe(0, io)[0].startswith('k_conv_bf16r') and not op.describe(1, io)[0].startswith('k_conv_bf16r'))
    key = (li, 'w', nb) if shared else (li, opcode, nb)         # nb separates the F(2x2,4x4) / F(3x3,4x4) transforms of the stride-1 layer
    if key in ucache:
        return ucache[key], True
    if isinstance(ucache, UCache):
        ucache[key] = ucache.buffer(key, nb, dev)
        if p_off is not None:
            ucache.log.append((key, op, opcode, io, p_off, nb))
    else:
        ucache[key] = torch.empty(nb, dtype=torch.uint8, device=dev)
    return ucache[key], False


def prefill_ucache(plan, flat, dev, pool=None):
    """A UCache holding every entry of `plan` (the log of an earlier UCache of the same network, input extent and storage mode),
    filled from the CURRENT weights `flat` by ONE pg_conv_prep_batch call: one launch per kernel family instead of one small weight
    transform / pack kernel per layer and direction.  Entries that end up unused cost a few microseconds; entries that are
    missing are made lazily by the conv calls as before."""
    uc = UCache(pool)
    if not plan or not PREP_BATCH:
        return uc
    items = (L.ConvPrepItem * len(plan))()
    for it, (key, op, opcode, io, p_off, nb) in zip(items, plan):
        buf = uc[key] = uc.buffer(key, nb, dev)
        it.g, it.op, it.algo, it.ws_bytes = op.g, opcode, op.algo | io, op.ws_arg
        it.P, it.u = L.ptr(flat, p_off), buf.data_ptr()
    uc.log = list(plan)
    L.check(L.load().pg_conv_prep_batch(len(plan), items, _stream()), 'pg_conv_prep_batch')
    return uc


def _dt(*views):
    """dtype mask of the *_t entry points: bit i = the i-th tensor argument is bf16."""
    m = 0
    for i, v in enumerate(views):
        if v is not None and v.bf:
            m |= 1 << i
    return m


def _pl(v):
    """(pointer, pixel stride) of an optional View argument: (NULL, 0) for None."""
    return (v.ptr(), v.ld) if v is not None else (None, 0)


def _in_check(y):
    if y.HW <= 1:
        raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                         f"torch.Size([{y.N}, {y.C}, {y.H}, {y.W}])")


def instnorm_act_fwd(y, out, stats, act, drop_p=0.0, seed=0):
    _in_check(y)
    ws = _workspace(int(L.load().pg_instnorm_workspace_bytes(y.N, y.HW, y.C)), y.t.device)
    L.check(L.load().pg_instnorm_act_fwd_t(y.ptr(), y.ld, out.ptr(), out.ld, stats.data_ptr(), y.N, y.HW, y.C, act, 1e-5,
                                           drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), _stream(), _dt(y, out)),
            'pg_instnorm_act_fwd')


class BNRun:
    """How the BatchNorm layers of one pass normalise -- chosen by module.training, not by Trainer.batch(train=...) (the reference
    calls .eval() only in its validation loop).  train: batch statistics per SEGMENT (nseg runs of N / nseg consecutive samples: the
    discriminator's pass over din[2N] stands for two calls of the reference, trainer.py:97,99), segment s's (mean, unbiased var) into
    the scratch at slot + s, folded into the running statistics later by bn_update_running in slot order.  eval: the running
    statistics of `bufs`, nothing is written.
    dist: the parallel.Dist of a SyncBatchNorm network while the data-parallel path is on (else None) -- a training-mode pass then
    normalises with the statistics of the GLOBAL batch (global segment s = every rank's segment s): each layer's local fp64 moments
    are SUM-reduced across ranks between the reduce and the rest (_bn_allreduce), forward and backward."""
    __slots__ = ('train', 'bufs', 'scratch', 'slot', 'nseg', 'dist')

    def __init__(self, train, bufs, scratch, slot=0, nseg=1, dist=None):
        self.train, self.bufs, self.scratch, self.slot, self.nseg = bool(train), bufs, scratch, slot, nseg if train else 1
        self.dist = dist if (train and dist is not None and dist.on) else None
        assert slot + self.nseg <= BN_SLOTS

    @property
    def world(self):
        """Ranks whose samples one segment's statistics are taken over."""
        return self.dist.world if self.dist is not None else 1


def _bn_check(y, nseg, world=1):
    if (y.N // nseg) * world * y.HW <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"torch.Size([{y.N // nseg * world}, {y.C}, {y.H}, {y.W}])")


def _bn_allreduce(dist, mom):
    """SUM of one layer's moments across ranks: on the comm stream behind the kernel that wrote them, and the consuming stream waits
    for it at once (the next kernel reads them) -- no host round trip.  Issued in layer order, the same on every rank."""
    dist.all_reduce_side(mom)()


def _bn_sync_fwd(lib, l, bn, flat, y, out, act, drop_p, seed, part, chunks, coef, st):
    """The split route of batchnorm_act_fwd: local moments -> all-reduce -> coefficients from the global moments -> apply."""
    w, b = L.ptr(flat, l.g_off), L.ptr(flat, l.be_off)
    mom = torch.empty(bn.nseg * y.C * 2, dtype=torch.float64, device=y.t.device)
    if part is not None:
        L.check(lib.pg_batchnorm_moments_fwd(None, y.ld, part.data_ptr(), chunks, mom.data_ptr(), y.N, y.HW, y.C, bn.nseg, None, 0, st),
                'pg_batchnorm_moments_fwd')
    else:
        ws = _workspace(int(lib.pg_batchnorm_workspace_bytes(y.N, y.HW, y.C, bn.nseg)), y.t.device)
        L.check(lib.pg_batchnorm_moments_fwd(y.ptr(), y.ld, None, 0, mom.data_ptr(), y.N, y.HW, y.C, bn.nseg, ws.data_ptr(), ws.numel(),
                                             st), 'pg_batchnorm_moments_fwd')
    _bn_allreduce(bn.dist, mom)
    count = float((y.N // bn.nseg) * bn.dist.world * y.HW)
    bstat = L.ptr(bn.scratch, l.bs_off + bn.slot * y.C * 2)
    L.check(lib.pg_batchnorm_coef_from_moments(mom.data_ptr(), count, w, b, BN_EPS, coef.data_ptr(), bstat, y.C, bn.nseg, st),
            'pg_batchnorm_coef_from_moments')
    L.check(lib.pg_batchnorm_act_apply(y.ptr(), y.ld, out.ptr(), out.ld, coef.data_ptr(), y.N, y.HW, y.C, bn.nseg, act, drop_p,
                                       seed & _MASK64, st), 'pg_batchnorm_act_apply')
    return coef


def batchnorm_act_fwd(l, bn, flat, y, out, act, drop_p=0.0, seed=0, part=None, chunks=0):
    """y -> BatchNorm2d of layer l -> activation -> dropout into out.  Returns the per-(segment, channel) coefficients it normalised
    with: a tensor of the pass's own, which the backward reads (a later running-statistics update cannot change it)."""
    lib = L.load()
    coef = torch.empty(bn.nseg * y.C * 4, dtype=torch.float32, device=y.t.device)
    w, b = L.ptr(flat, l.g_off), L.ptr(flat, l.be_off)
    st = _stream()
    if not bn.train:
        L.check(lib.pg_batchnorm_eval_coef(L.ptr(bn.bufs, l.rm_off), L.ptr(bn.bufs, l.rv_off), w, b, y.C, BN_EPS, coef.data_ptr(), st),
                'pg_batchnorm_eval_coef')
        L.check(lib.pg_batchnorm_act_apply(y.ptr(), y.ld, out.ptr(), out.ld, coef.data_ptr(), y.N, y.HW, y.C, 1, act, drop_p,
                                           seed & _MASK64, st), 'pg_batchnorm_act_apply')
        return coef
    _bn_check(y, bn.nseg, bn.world)
    if bn.dist is not None:
        return _bn_sync_fwd(lib, l, bn, flat, y, out, act, drop_p, seed, part, chunks, coef, st)
    bstat = L.ptr(bn.scratch, l.bs_off + bn.slot * y.C * 2)
    if part is not None:
        L.check(lib.pg_batchnorm_stats(None, y.ld, part.data_ptr(), chunks, w, b, coef.data_ptr(), bstat, y.N, y.HW, y.C, bn.nseg,
                                       BN_EPS, None, 0, st), 'pg_batchnorm_stats')
        L.check(lib.pg_batchnorm_act_apply(y.ptr(), y.ld, out.ptr(), out.ld, coef.data_ptr(), y.N, y.HW, y.C, bn.nseg, act, drop_p,
                                           seed & _MASK64, st), 'pg_batchnorm_act_apply')
        return coef
    ws = _workspace(int(lib.pg_batchnorm_workspace_bytes(y.N, y.HW, y.C, bn.nseg)), y.t.device)
    L.check(lib.pg_batchnorm_act_fwd(y.ptr(), y.ld, out.ptr(), out.ld, w, b, coef.data_ptr(), bstat, y.N, y.HW, y.C, bn.nseg, act,
                                     BN_EPS, drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), st), 'pg_batchnorm_act_fwd')
    return coef


def batchnorm_act_bwd(l, train, nseg, gflat, g1, g2, y, coef, dy, act, drop_p=0.0, seed=0, dist=None):
    """Backward of batchnorm_act_fwd (train / nseg / dist: those of its pass).  gflat None: no weight / bias gradients (the generator
    step's pass through D); else they are WRITTEN into gflat.  dist (a training-mode pass that normalised with the global batch's
    statistics): the split route -- local moments -> all-reduce -> apply with the global count; the weight / bias gradients stay the
    LOCAL sums (the flat gradient is SUM-reduced across ranks afterwards like every other parameter's)."""
    lib = L.load()
    nseg = nseg if train else 1
    ws = _workspace(int(lib.pg_batchnorm_workspace_bytes(y.N, y.HW, y.C, nseg)), y.t.device)
    dw, db = (L.ptr(gflat, l.g_off), L.ptr(gflat, l.be_off)) if gflat is not None else (None, None)
    if train and dist is not None:
        st = _stream()
        g2p, g2l = _pl(g2)
        mom = torch.empty(nseg * y.C * 2, dtype=torch.float64, device=y.t.device)
        L.check(lib.pg_batchnorm_moments_bwd(g1.ptr(), g1.ld, g2p, g2l, y.ptr(), y.ld, coef.data_ptr(), mom.data_ptr(), dw, db, y.N, y.HW,
                                             y.C, nseg, act, drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), st),
                'pg_batchnorm_moments_bwd')
        _bn_allreduce(dist, mom)
        count = float((y.N // nseg) * dist.world * y.HW)
        L.check(lib.pg_batchnorm_bwd_apply(g1.ptr(), g1.ld, g2p, g2l, y.ptr(), y.ld, coef.data_ptr(), mom.data_ptr(), count, dy.ptr(),
                                           dy.ld, y.N, y.HW, y.C, nseg, act, drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), st),
                'pg_batchnorm_bwd_apply')
        return
    L.check(lib.pg_batchnorm_act_bwd(g1.ptr(), g1.ld, *_pl(g2), y.ptr(), y.ld, coef.data_ptr(), dy.ptr(), dy.ld, dw, db, y.N, y.HW, y.C,
                                     nseg, 1 if train else 0, act, drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), _stream()),
            'pg_batchnorm_act_bwd')


def bn_update_running(layers, bufs, counters, scratch, nslots):
    """Fold the batch statistics in slots [0, nslots) of every BatchNorm layer into its running statistics, in slot order, and add
    nslots to its num_batches_tracked: ONE launch per network."""
    bl = [l for l in layers if l.bn]
    if not bl:
        return
    items = (L.BnUpdateItem * len(bl))()
    for it, l in zip(items, bl):
        it.bstat, it.C = L.ptr(scratch, l.bs_off), l.cout
        it.running_mean, it.running_var = L.ptr(bufs, l.rm_off), L.ptr(bufs, l.rv_off)
        it.num_batches_tracked = L.ptr(counters, l.bn_idx)
    L.check(L.load().pg_batchnorm_update_running(len(bl), items, nslots, BN_MOMENTUM, _stream()), 'pg_batchnorm_update_running')


def _exp_env(name, default='1'):
    """A/B switches for same-device timing: honoured only when PATCHGAN_EXPERIMENT is set (like the C side's pg_exp_env)."""
    return os.environ.get(name, default) if 'PATCHGAN_EXPERIMENT' in os.environ else default


FUSE_IN_STATS = _exp_env('PATCHGAN_FUSE_IN_STATS') != '0'     # InstanceNorm sums from the producing conv
KEEP_V = _exp_env('PATCHGAN_KEEP_V') != '0'                   # transformed input handed from forward to weight gradient
CACHE_U = _exp_env('PATCHGAN_CACHE_U') != '0'                 # per-step cache of transformed / packed discriminator weights
PREP_BATCH = _exp_env('PATCHGAN_PREP_BATCH') != '0'           # one batched weight-preparation launch per network and step
FUSE_ACT_BWD = _exp_env('PATCHGAN_FUSE_ACT_BWD') != '0'       # activation backward in the data-gradient epilogue above it
SEAM8 = _exp_env('PATCHGAN_SEAM8') != '0'       # bf16 storage: image-facing tensors in 8-channel bf16 pixels
WGRAD_SIDE = _exp_env('PATCHGAN_WGRAD_SIDE') != '0'       # weight gradients of a backward pass on a second stream (Exec)
BF16_WGRAD_SIDE = _exp_env('PATCHGAN_BF16_WGRAD_SIDE') != '0'       # bf16 networks' weight gradients on the second stream too (round 5: noise, off; round 6: cfg4 5.41 -> 5.35 ms, cfg2-bf16 3.41 -> 3.33 in three alternating runs each: on)
SHARE_DY_V = _exp_env('PATCHGAN_SHARE_DY_V') != '0'       # ... and the two halves share the transformed dy (A/B switch)
SPLIT_BWD_BIG = _exp_env('PATCHGAN_SPLIT_BWD_BIG') != '0'       # with the second stream: the decoder's fused backward call as its two halves (8.83 -> 8.65 ms at cfg2)


def instnorm_act_bwd(g1, g2, y, stats, dy, act, drop_p=0.0, seed=0):
    ws = _workspace(int(L.load().pg_instnorm_workspace_bytes(y.N, y.HW, y.C)), y.t.device)
    L.check(L.load().pg_instnorm_act_bwd_t(g1.ptr(), g1.ld, *_pl(g2), y.ptr(), y.ld, stats.data_ptr(), dy.ptr(), dy.ld,
                                           y.N, y.HW, y.C, act, drop_p, seed & _MASK64, ws.data_ptr(), ws.numel(), _stream(),
                                           _dt(g1, g2, y, dy)), 'pg_instnorm_act_bwd')


def instnorm_affine_act_fwd(y, out, stats, flat, g_off, be_off, act, drop_p=0.0, seed=0, part=None, chunks=0):
    """instnorm_act_fwd with the per-channel scale / shift at g_off / be_off of `flat` (nn.InstanceNorm2d(affine=True)); part / chunks:
    the statistics come from a conv epilogue's partial sums."""
    _in_check(y)
    lib = L.load()
    w, b = L.ptr(flat, g_off), L.ptr(flat, be_off)
    if part is not None:
        L.check(lib.pg_instnorm_affine_act_fwd_parts_t(y.ptr(), y.ld, out.ptr(), out.ld, w, b, stats.data_ptr(), part.data_ptr(), chunks,
                                                       y.N, y.HW, y.C, act, 1e-5, drop_p, seed & _MASK64, _stream(), _dt(y, out)),
                'pg_instnorm_affine_act_fwd_parts')
        return
    ws = _workspace(int(lib.pg_instnorm_affine_workspace_bytes(y.N, y.HW, y.C)), y.t.device)
    L.check(lib.pg_instnorm_affine_act_fwd_t(y.ptr(), y.ld, out.ptr(), out.ld, w, b, stats.data_ptr(), y.N, y.HW, y.C, act, 1e-5, drop_p,
                                             seed & _MASK64, ws.data_ptr(), ws.numel(), _stream(), _dt(y, out)),
            'pg_instnorm_affine_act_fwd')


def instnorm_affine_act_bwd(g1, g2, y, stats, dy, flat, gflat, g_off, be_off, act, drop_p=0.0, seed=0):
    """Backward of instnorm_affine_act_fwd.  gflat None: no scale / shift gradients; else they are WRITTEN at g_off / be_off of it."""
    lib = L.load()
    ws = _workspace(int(lib.pg_instnorm_affine_workspace_bytes(y.N, y.HW, y.C)), y.t.device)
    dw, db = (L.ptr(gflat, g_off), L.ptr(gflat, be_off)) if gflat is not None else (None, None)
    L.check(lib.pg_instnorm_affine_act_bwd_t(g1.ptr(), g1.ld, *_pl(g2), y.ptr(), y.ld, L.ptr(flat, g_off), L.ptr(flat, be_off),
                                             stats.data_ptr(), dy.ptr(), dy.ld, dw, db, y.N, y.HW, y.C, act, drop_p, seed & _MASK64,
                                             ws.data_ptr(), ws.numel(), _stream(), _dt(g1, g2, y, dy)), 'pg_instnorm_affine_act_bwd')


def act_bwd(g1, g2, a, dy, act):
    L.check(L.load().pg_act_bwd_t(g1.ptr(), g1.ld, *_pl(g2), *_pl(a), dy.ptr(), dy.ld, dy.npix, dy.C, act, 0.0, 0, _stream(),
                                  _dt(g1, g2, a, dy)), 'pg_act_bwd')


def softmax_fwd(y, out):
    L.check(L.load().pg_softmax_fwd(y.ptr(), y.ld, out.ptr(), out.ld, y.npix, y.C, _stream()), 'pg_softmax_fwd')


def softmax_bwd(g1, g2, out, dy):
    L.check(L.load().pg_softmax_bwd(g1.ptr(), g1.ld, *_pl(g2), out.ptr(), out.ld, dy.ptr(), dy.ld, dy.npix, dy.C, _stream()),
            'pg_softmax_bwd')


def adam_scalars(step, lr, beta1=0.9, beta2=0.999, weight_decay=None):
    """(lr / bc1, sqrt(bc2)) as the float32 values pg_adam_step forms from its arguments: what pg_adam_step_dev reads from device memory.
    With a weight_decay also decay_mul(lr, weight_decay), the third float pg_adamw_step_dev reads."""
    bc1 = np.float32(1.0 - beta1 ** step)
    sc = np.float32(lr) / bc1, np.float32(math.sqrt(1.0 - beta2 ** step))
    return sc if weight_decay is None else sc + (np.float32(decay_mul(lr, weight_decay)),)


def _is_number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float, np.floating, np.integer))


def _one_or_pair(value, one, msg):
    """A per-network setting as (gen, disc): None -> (None, None), one number -> one(number) for both, a pair whose members may be
    None -> one(member) of each; ValueError(msg) for a sequence of another length."""
    if value is None:
        return None, None
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(msg)
        return tuple(None if x is None else one(x) for x in value)
    x = one(value)
    return x, x


def check_ema_decay(decay):
    """The decay of the generator's weight average as a float in [0, 1), or ValueError (what pg_adam_ema_step accepts)."""
    if not _is_number(decay):
        raise ValueError(f"ema_decay must be None or a float in [0, 1), not {decay!r}")
    d = float(decay)
    if not (0.0 <= d < 1.0) or not (float(np.float32(d)) < 1.0):        # (the kernel takes it as a float32)
        raise ValueError(f"ema_decay must be None or a float in [0, 1), not {decay!r}")
    return d


def check_clip_norm(value):
    """Trainer.clip_grad_norm as (gen_max_norm, disc_max_norm), each None or a float > 0 (inf allowed: monitor only), or ValueError.
    `value`: None, one positive number for both networks, or a pair whose members may be None (what pg_grad_norm accepts)."""
    msg = f"clip_grad_norm must be None, a positive float or a pair of them (members may be None), not {value!r}"

    def one(x):
        if not _is_number(x) or not float(x) > 0.0:          # (a NaN fails the comparison)
            raise ValueError(msg)
        return float(x)
    return _one_or_pair(value, one, msg)


# struct pg_grad_stat (include/patchgan_hip.h): one 64-byte status block per network, read on the host as one record
GRAD_STAT = np.dtype([('norm', '<f4'), ('coef', '<f4'), ('apply', '<u4'), ('reserved', '<u4'), ('steps', '<u8'), ('clipped', '<u8'),
                      ('skipped', '<u8'), ('max_norm', '<f8'), ('sum_norm', '<f8'), ('sumsq', '<f8')])
assert GRAD_STAT.itemsize == 64


def grad_norm_workspace_bytes(n):
    return L.load().pg_grad_norm_workspace_bytes(n)


def grad_norm(g, max_norm, ws, stat):
    """The 2-norm of the flat fp32 gradient `g` (fp64 sum of squares, fixed order) and the clipping coefficient for `max_norm` into the
    device status block `stat` (64 bytes: GRAD_STAT); `ws`: grad_norm_workspace_bytes(g.numel()) bytes.  Two launches on the current
    stream, no host read."""
    L.check(L.load().pg_grad_norm(g.data_ptr(), g.numel(), max_norm, ws.data_ptr(), ws.numel() * ws.element_size(), stat.data_ptr(),
                                  _stream()), 'pg_grad_norm')


_BETAS_MSG = "betas must be None, a pair (beta1, beta2) of floats in [0, 1) or a pair of such pairs (generator, discriminator), not {!r}"
_WD_MSG = "weight_decay must be None, a finite number >= 0 or a pair of them (generator, discriminator; members may be None), not {!r}"


def check_betas(value):
    """Trainer.betas as ((gen_beta1, gen_beta2), (disc_beta1, disc_beta2)), or ValueError.  `value`: None (torch.optim.Adam's
    (0.9, 0.999) for both networks), one pair for both, or a pair of pairs; every beta a float in [0, 1) that stays below 1 as a
    float32 (what pg_adam_step* and pg_adamw_step* take)."""
    def pair(x):
        if not isinstance(x, (tuple, list)) or len(x) != 2 or not all(_is_number(b) for b in x):
            raise ValueError(_BETAS_MSG.format(value))
        x = tuple(float(b) for b in x)
        if not all(0.0 <= b < 1.0 and float(np.float32(b)) < 1.0 for b in x):          # (a NaN fails the comparison)
            raise ValueError(_BETAS_MSG.format(value))
        return x
    if value is None:
        return (0.9, 0.999), (0.9, 0.999)
    if isinstance(value, (tuple, list)) and len(value) == 2 and all(isinstance(x, (tuple, list)) for x in value):
        return pair(value[0]), pair(value[1])
    both = pair(value)
    return both, both


def check_weight_decay(value):
    """Trainer.weight_decay as (gen, disc), each None (the network takes the entry points without a decay) or a float > 0, or
    ValueError.  `value`: None, one finite number >= 0 for both networks, or a pair whose members may be None; 0 counts as None."""
    def one(x):
        if not _is_number(x) or not (0.0 <= float(x) < float('inf')):          # (a NaN fails the comparison)
            raise ValueError(_WD_MSG.format(value))
        return float(x) or None
    return _one_or_pair(value, one, _WD_MSG.format(value))


def decay_mul(lr, weight_decay):
    """1 - lr * weight_decay formed in double: torch.optim.AdamW's param.mul_(1 - lr * weight_decay); pg_adamw_step takes it rounded
    once to a float32, which must land in (0, 1].  ValueError for lr * weight_decay >= 1 (the decay would flip or zero the weights)."""
    dm = 1.0 - float(lr) * float(weight_decay)
    if not (dm > 0.0 and 0.0 < float(np.float32(dm)) <= 1.0):
        raise ValueError(f"lr * weight_decay must be < 1 (lr = {lr!r}, weight_decay = {weight_decay!r})")
    return dm


def adam_entry(ema, stat, weight_decay, dev):
    """The library entry point of an Adam update from four booleans: is there a weight average, a clipping status block, a decoupled
    weight decay, and do the step-dependent scalars come from device memory (a step being captured)."""
    name = 'pg_adamw_step' if weight_decay else 'pg_adam_clip_step' if stat else 'pg_adam_ema_step' if ema else 'pg_adam_step'
    return name + '_dev' if dev else name


def adam_update(p, g, m, v, *, step=None, lr=None, scalars=None, ema=None, ema_decay=None, stat=None, weight_decay=None, beta1=0.9,
                beta2=0.999, eps=1e-8):
    """One fused Adam pass over the flat fp32 buffers p, g, m, v on the current stream: torch.optim.Adam (reference trainer.py:169-172),
    bias corrections in Python doubles like torch.  Either `step` and `lr`, or `scalars`: a device tensor holding adam_scalars(...) -- a
    launch without step-dependent arguments, what a captured step replays.  Options, each None for off, all in the same pass:
    `ema` (+ `ema_decay`): ema += (p_new - ema) * (1 - ema_decay), the weights' exponential moving average; `stat`: the update runs on
    g * coef, coef and the skip flag read from the status block grad_norm wrote; `weight_decay`: on p * decay_mul(lr, weight_decay),
    torch.optim.AdamW's decoupled decay (with `scalars` the multiplier is their third float).  adam_entry names the entry point."""
    dev = scalars is not None
    if (step is None) != (lr is None) or dev == (step is not None):
        raise ValueError("adam_update takes either step and lr or scalars")
    name = adam_entry(ema is not None, stat is not None, weight_decay is not None, dev)
    plain = name.startswith('pg_adam_step')
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()]
    if not plain:
        args.append(ema.data_ptr() if ema is not None else None)
    args.append(p.numel())
    if dev:
        args += [beta1, beta2, eps, scalars.data_ptr()]
    else:
        args += [lr, beta1, beta2, eps, 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)]
        if weight_decay is not None:
            args.append(decay_mul(lr, weight_decay))
    if not plain:
        args.append(ema_decay if ema is not None else 0.0)
    if stat is not None or weight_decay is not None:
        args.append(stat.data_ptr() if stat is not None else None)
    L.check(getattr(L.load(), name)(*args, _stream()), name)


def check_accumulate(value):
    """Trainer.accumulate / train_params.accumulate as the window length: None (off: None or 1) or an int >= 2, or ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"accumulate must be None or an int >= 1 (micro-batches per optimizer step), not {value!r}")
    return int(value) if value >= 2 else None


def accum_phase(done, k):
    """The phase of the training call that follows `done` completed calls of a window of k >= 2: 'begin' | 'add' | 'close'."""
    if not 0 <= done < k:
        raise ValueError(f"window position {done} outside [0, {k})")
    return 'begin' if done == 0 else ('close' if done + 1 == k else 'add')


def accum_scale(count):
    """1 / count as pg_grad_accum's closing modes take it: formed in double, rounded once."""
    return np.float32(1.0 / count)


ACC_MODES = {'begin': L.ACC_BEGIN, 'add': L.ACC_ADD, 'close': L.ACC_CLOSE, 'close_only': L.ACC_CLOSE_ONLY}


def grad_accum(acc, g, mode, scale=1.0):
    """One pass of pg_grad_accum over the flat fp32 accumulator `acc` and gradient `g` on the current stream.  mode 'begin': acc = g;
    'add': acc += g; 'close': g = (acc + g) * scale; 'close_only': g = acc * scale (scale = accum_scale(count); the first two ignore it)."""
    L.check(L.load().pg_grad_accum(acc.data_ptr(), g.data_ptr(), g.numel(), ACC_MODES[mode], float(scale), _stream()), 'pg_grad_accum')


def seg_confusion(p, y, threshold, counts):
    """Add the confusion counts of prediction View p against target View y (fp32, the same shape) to `counts`: an int64 device tensor
    of K*K + 1 words, K = 2 for one channel (p >= threshold against y >= 0.5) and the channel count otherwise (first maximum against
    first maximum; a pixel without a positive target channel counts as ignored in the last word).  pg_seg_confusion, on the current
    stream; nothing is read back (metrics.SegCounts.read does that, once per pass)."""
    assert (p.N, p.H, p.W, p.C) == (y.N, y.H, y.W, y.C) and not p.bf and not y.bf, 'seg_confusion takes fp32 views of one shape'
    K = 2 if p.C == 1 else p.C
    assert counts.dtype == torch.int64 and counts.numel() == K * K + 1 and counts.is_contiguous() and counts.device == p.t.device
    L.check(L.load().pg_seg_confusion(p.ptr(), p.ld, y.ptr(), y.ld, p.N, p.HW, p.C, float(threshold), counts.data_ptr(), _stream()),
            'pg_seg_confusion')


def seg_hist(p, y, bins, hist):
    """Add the per-class prediction histograms of View p against target View y (fp32, the same shape) to `hist`: an int64 device tensor
    of C*2*bins + 1 words, [channel][label][bin] and the ignored pixels in the last word (metrics.SegHist; bins a power of two in
    16..1024, C * bins <= 8192).  pg_seg_hist, on the current stream; nothing is read back."""
    assert (p.N, p.H, p.W, p.C) == (y.N, y.H, y.W, y.C) and not p.bf and not y.bf, 'seg_hist takes fp32 views of one shape'
    bins = int(bins)
    assert hist.dtype == torch.int64 and hist.numel() == p.C * 2 * bins + 1 and hist.is_contiguous() and hist.device == p.t.device
    L.check(L.load().pg_seg_hist(p.ptr(), p.ld, y.ptr(), y.ld, p.N, p.HW, p.C, bins, hist.data_ptr(), _stream()), 'pg_seg_hist')


TTA_VARIANTS = {None: 1, 'hflip': 2, 'flips': 4, 'd4': 8}


def tta_variants(tta):
    """Number K of test-time-augmentation variants per tile: None 1, 'hflip' 2 (horizontal flip), 'flips' 4 (both flips), 'd4' 8 (the
    dihedral group).  Variant k is transpose(-1, -2) if k & 4, then flip(-2) if k & 2, then flip(-1) if k & 1."""
    if not (tta is None or isinstance(tta, str)) or tta not in TTA_VARIANTS:
        raise ValueError(f"tta must be None, 'hflip', 'flips' or 'd4', not {tta!r}")
    return TTA_VARIANTS[tta]


AUG_POLICIES = {'flip': L.AUG_FLIP, 'translation': L.AUG_TRANSLATION, 'cutout': L.AUG_CUTOUT}


def diffaug_policy(policy):
    """The PG_AUG_* bits of a differentiable-augmentation policy: None, a comma-separated string or a sequence of names out of
    'flip', 'translation', 'cutout' (the order of application is fixed: flip, translation, cutout).  The empty policy equals None:
    0.  ValueError for anything else, naming the allowed words."""
    if policy is None:
        return 0
    if isinstance(policy, str):
        names = [w.strip() for w in policy.split(',') if w.strip()]
    elif isinstance(policy, (list, tuple)):
        names = list(policy)
    else:
        names = [policy]
    bits = 0
    for w in names:
        if not isinstance(w, str) or w not in AUG_POLICIES:
            raise ValueError(f"diffaug must be None or made of {', '.join(AUG_POLICIES)} (a comma-separated string or a list), not {policy!r}")
        bits |= AUG_POLICIES[w]
    return bits


def diffaug_seed(seed):
    """Trainer.diffaug_seed checked: an int in 0 .. 2^64 - 1 (bool excluded).  ValueError otherwise."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _MASK64:
        raise ValueError(f"diffaug_seed must be an integer in 0 .. 2**64 - 1, not {seed!r}")
    return int(seed)


def diffaug_params(seed, counter, step, policy, sample0, N, H, W, params=None, device=None):
    """The parameter table of one step (pg_diffaug_params): an int32 device tensor [N, 8], rows {flip, ty, tx, cut_top, cut_left, cut_h,
    cut_w, 0} of global samples sample0 .. sample0 + N.  `counter`: a one-word int64 device tensor holding the step count, advanced by
    the launch -- or None, then the host value `step` is the step count.  `policy`: PG_AUG_* bits.  On the current stream."""
    if params is None:
        params = torch.empty(N, 8, dtype=torch.int32, device=counter.device if counter is not None else device)
    assert params.dtype == torch.int32 and params.is_contiguous() and params.numel() == N * 8
    assert counter is None or (counter.dtype == torch.int64 and counter.numel() == 1 and counter.device == params.device)
    L.check(L.load().pg_diffaug_params(int(seed) & _MASK64, counter.data_ptr() if counter is not None else None, int(step) & _MASK64,
                                       int(policy), int(sample0), N, H, W, params.data_ptr(), _stream()), 'pg_diffaug_params')
    return params


def _diffaug_rows(view, params, n0):
    assert not view.bf, 'the augmentation moves fp32 views'
    assert params.dtype == torch.int32 and params.is_contiguous() and params.dim() == 2 and params.shape[1] == 8
    assert 0 <= n0 and n0 + view.N <= params.shape[0], (n0, view.N, tuple(params.shape))
    return params.data_ptr() + n0 * 32


def diffaug_fwd(src, dst, params, n0=0):
    """dst = T(src) for fp32 Views of one shape (pg_diffaug_fwd); sample i of the views takes row n0 + i of the table -- a half of a
    2N buffer is passed as View.samples(...) with the rows of the samples it pairs with.  On the current stream."""
    assert (src.N, src.H, src.W, src.C) == (dst.N, dst.H, dst.W, dst.C) and not dst.bf
    L.check(L.load().pg_diffaug_fwd(src.ptr(), src.ld, dst.ptr(), dst.ld, _diffaug_rows(src, params, n0), src.N, src.H, src.W, src.C,
                                    _stream()), 'pg_diffaug_fwd')
    return dst


def diffaug_bwd(g, dsrc, params, n0=0):
    """dsrc = T^t(g), the exact adjoint of diffaug_fwd with the same rows (pg_diffaug_bwd): every element of dsrc is written."""
    assert (g.N, g.H, g.W, g.C) == (dsrc.N, dsrc.H, dsrc.W, dsrc.C) and not dsrc.bf
    L.check(L.load().pg_diffaug_bwd(g.ptr(), g.ld, dsrc.ptr(), dsrc.ld, _diffaug_rows(g, params, n0), g.N, g.H, g.W, g.C, _stream()),
            'pg_diffaug_bwd')
    return dsrc


def window_table(window, size):
    """The blend window as `size` float64 weights: None (uniform) ones, 'pyramid' min(u + 1, size - u), 'hann' the half-sample
    sin^2 form (positive everywhere), or a 1-D sequence of `size` numbers.  A pixel may be covered by a single tile, so every weight
    must be finite and > 0: ValueError otherwise, and for an unknown name or a wrong length."""
    if window is None:
        return np.ones(size, dtype=np.float64)
    if isinstance(window, str):
        if window == 'pyramid':
            u = np.arange(size)
            return np.minimum(u + 1, size - u).astype(np.float64)
        if window == 'hann':
            return np.sin(np.pi * (np.arange(size) + 0.5) / size) ** 2
        raise ValueError(f"window must be None, 'pyramid', 'hann' or a sequence of {size} weights, not {window!r}")
    try:
        table = np.array(window, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"window must be None, 'pyramid', 'hann' or a sequence of {size} weights, not {window!r}") from None
    if table.ndim != 1 or table.shape[0] != size:
        raise ValueError(f"a window for {size}x{size} tiles is a 1-D sequence of {size} weights, not of shape {table.shape}")
    if not (np.isfinite(table).all() and (table > 0).all()):
        raise ValueError("every window weight must be finite and > 0 (a pixel may be covered by a single tile)")
    return table


_WINDOWS = {}


def window_dev(window, size, device):
    """window_table on the device, uploaded once per (window, size, device)."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    named = window is None or isinstance(window, str)
    table = None if named else window_table(window, size)
    key = (window if named else table.tobytes(), size, device)
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.from_numpy(window_table(window, size) if named else table).to(device)
    return _WINDOWS[key]


def tiles_gather(image, size, overlap, tta=None):
    """reference infer.py:14-35 (n_crop): device image [C, H, W] -> View of the ny*nx overlapping size x size tiles in the
    NHWC batch layout the generator kernels read.  tta ('hflip' / 'flips' / 'd4', tta_variants): K variants of every tile, variant k
    of tile t at sample k * ny*nx + t."""
    C, H, W = image.shape
    eff = int(overlap * size)
    lib = L.load()
    K = tta_variants(tta)
    ny, nx = lib.pg_tiles_count(H, size, eff), lib.pg_tiles_count(W, size, eff)
    if ny <= 0 or nx <= 0:
        raise ValueError(f"cannot cut {size}x{size} tiles with overlap {overlap} from a {H}x{W} image")
    image = image.to(dtype=torch.float32).contiguous()
    tiles = View.alloc(K * ny * nx, size, size, C, image.device)
    if tta is None:
        L.check(lib.pg_tiles_gather(image.data_ptr(), C, H, W, size, eff, tiles.ptr(), tiles.ld, _stream()), 'pg_tiles_gather')
    else:
        L.check(lib.pg_tiles_gather_tta(image.data_ptr(), C, H, W, size, eff, K, tiles.ptr(), tiles.ld, _stream()),
                'pg_tiles_gather_tta')
    return tiles


def tiles_blend(tiles, image_size, threshold, overlap, tta=None, window=None):
    """reference infer.py:38-68 (build_mask): View of predicted tiles -> overlap-averaged mask on the device: float64
    [H, W] for one class, int64 class index [H, W] for several (same values / dtypes as the reference returns).  With tta and / or
    window (window_table): the K variants of a tile read back through the inverse map, each tile weighed by window[y] * window[x]."""
    H, W = image_size
    size = tiles.H
    eff = int(overlap * size)
    lib = L.load()
    K = tta_variants(tta)
    if K * lib.pg_tiles_count(H, size, eff) * lib.pg_tiles_count(W, size, eff) != tiles.N or tiles.W != size:
        raise ValueError(f"{tiles.N} tiles of {tiles.H}x{tiles.W} do not tile a {H}x{W} image with overlap {overlap}"
                         + (f" in {K} variants" if K > 1 else ""))
    dev = tiles.t.device
    table = None if tta is None and window is None else window_dev(window, size, dev)
    if tiles.C > 1:
        out = torch.empty(H, W, dtype=torch.int64, device=dev)
        mask_p, arg_p = None, out.data_ptr()
    else:
        out = torch.empty(H, W, dtype=torch.float64, device=dev)
        mask_p, arg_p = out.data_ptr(), None
    if table is None:
        L.check(lib.pg_tiles_blend(tiles.ptr(), tiles.ld, tiles.C, size, eff, H, W, float(threshold), mask_p, arg_p, _stream()),
                'pg_tiles_blend')
    else:
        L.check(lib.pg_tiles_blend_win(tiles.ptr(), tiles.ld, tiles.C, size, eff, H, W, K, table.data_ptr(), float(threshold), mask_p,
                                       arg_p, _stream()), 'pg_tiles_blend_win')
    return out


_GOLD = 0x9E3779B97F4A7C15


def _shift_seed(seed, elem_offset):
    """Seed whose dropout stream is `seed`'s shifted by elem_offset elements: pg_dropout_keep hashes
    seed + GOLD * (e + 1), so the mask of local element e under the shifted seed is the mask of global element
    e + elem_offset under `seed` (data parallelism: rank r's samples sit at r*N.. of the global batch)."""
    return (seed + _GOLD * elem_offset) & _MASK64


def _mix_seed(base, *vals):
    h = (base * 0x9E3779B97F4A7C15 + 0x1234567) & _MASK64
    for v in vals:
        h ^= (v + 0x9E3779B97F4A7C15 + ((h << 6) & _MASK64) + (h >> 2)) & _MASK64
        h = (h * 0xBF58476D1CE4E5B9) & _MASK64
    return h


# ------------------------------------------------------------------------------------------------
# the norm blocks of a pass
# ------------------------------------------------------------------------------------------------


class NormPass:
    """The norm blocks of ONE pass through a network (InstanceNorm, plain or affine per layer -- LayerSpec.in_affine --, here, BatchNorm
    below): which normalisation a layer has, where its statistics come from and what its backward needs is decided in this class and
    nowhere else.  norm_pass() builds it at the top of a
    forward pass and the context carries it to the backward.  The engines hand a block's tensors over and keep what its forward
    returns (c.stats[i] / c.statsd[i]) without looking at it: InstanceNorm's [N*C*2] fp32 (mean, rstd), BatchNorm's coefficients.
    train / seed / sample0: the dropout behind the generator's blocks (GeneratorEngine.forward).  A block's `key` is its place in the
    dropout stream, (1 encoder | 2 decoder, index); None: a block without dropout (the discriminator's)."""
    conv_sums = True          # the statistics are the batch's own: take them from the producing conv's epilogue where it emits them

    def __init__(self, train=False, seed=0, sample0=0):
        self.train, self.seed, self.sample0 = train, seed, sample0

    def _dropout(self, l, key, y):
        """(probability, seed) of the dropout behind block `key`: the masks are those of the global batch (_shift_seed)."""
        if key is None:
            return 0.0, 0
        return (0.2 if (self.train and l.dropout) else 0.0), _shift_seed(_mix_seed(self.seed, *key), self.sample0 * y.HW * y.C)

    def conv_norm_act(self, op, opcode, src, flat, l, key, y, out, act, v_keep=None, u_cache=None, u_valid=False):
        """Conv2d / ConvTranspose2d (no bias) -> norm -> activation -> dropout (unet.py:19-30,53-67).  Where the conv's kernel can
        emit the per-sample sums of its output (polyphase Winograd output transform) the statistics come from those partials and the
        separate statistics pass over y is skipped.  Returns what backward() needs."""
        conv = op.big2small if opcode == 0 else op.small2big
        kw = {'v_keep': v_keep} if v_keep is not None else {}
        if u_cache is not None:
            kw.update(u_cache=u_cache, u_valid=u_valid)
        self._check(y)                # (torch raises from the norm; nothing is launched for a pass it would refuse)
        chunks = op.stats_chunks(opcode, src, y) if (FUSE_IN_STATS and self.conv_sums) else 0
        part = torch.empty(y.N * chunks * y.C * 2, dtype=torch.float64, device=y.t.device) if chunks else None
        conv(src, flat, l.p_off, None, 0, y, part=part, **kw)
        return self._norm_act(l, flat, y, out, act, *self._dropout(l, key, y), part, chunks)

    def norm_act(self, l, flat, y, out, act):
        """norm -> activation on a tensor that exists already (disc.py:31-32: Conv -> Tanh -> norm).  Returns what backward() needs."""
        return self._norm_act(l, flat, y, out, act, 0.0, 0, None, 0)

    def _check(self, y):
        _in_check(y)

    def _norm_act(self, l, flat, y, out, act, drop_p, seed, part, chunks):
        stats = torch.empty(y.N * y.C * 2, dtype=torch.float32, device=y.t.device)
        if l.in_affine:          # (the backward recomputes the forward's z: it is handed the scale / shift the forward read)
            instnorm_affine_act_fwd(y, out, stats, flat, l.g_off, l.be_off, act, drop_p, seed, part, chunks)
            return stats, flat
        if part is None:
            instnorm_act_fwd(y, out, stats, act, drop_p, seed)
        else:
            L.check(L.load().pg_instnorm_act_fwd_parts_t(y.ptr(), y.ld, out.ptr(), out.ld, stats.data_ptr(), part.data_ptr(), chunks, y.N,
                                                         y.HW, y.C, act, 1e-5, drop_p, seed & _MASK64, _stream(), _dt(y, out)),
                    'pg_instnorm_act_fwd_parts')
        return stats

    def backward(self, l, gflat, g1, g2, y, saved, dy, act, key=None):
        """dy = the gradient wrt the block's norm input y from g1 (+ g2) wrt its output; `saved`: what the forward returned.  A norm
        with parameters WRITES their gradients into gflat (None: not wanted, the generator step's pass through D)."""
        if l.in_affine:
            stats, flat = saved
            instnorm_affine_act_bwd(g1, g2, y, stats, dy, flat, gflat, l.g_off, l.be_off, act, *self._dropout(l, key, y))
        else:
            instnorm_act_bwd(g1, g2, y, saved, dy, act, *self._dropout(l, key, y))


class BatchNormPass(NormPass):
    """NormPass of a BatchNorm network under the pass's BNRun."""

    def __init__(self, bn, **dropout):
        super().__init__(**dropout)
        self.bn, self.conv_sums = bn, bn.train

    def _check(self, y):
        if self.bn.train:
            _bn_check(y, self.bn.nseg, self.bn.world)

    def _norm_act(self, l, flat, y, out, act, drop_p, seed, part, chunks):
        return batchnorm_act_fwd(l, self.bn, flat, y, out, act, drop_p, seed, part=part, chunks=chunks)

    def backward(self, l, gflat, g1, g2, y, saved, dy, act, key=None):
        bn = self.bn
        batchnorm_act_bwd(l, bn.train, bn.nseg, gflat, g1, g2, y, saved, dy, act, *self._dropout(l, key, y), dist=bn.dist)


def norm_pass(bn, **dropout):
    """The NormPass of a pass called with bn = its BNRun (a BatchNorm network) or None (InstanceNorm)."""
    return BatchNormPass(bn, **dropout) if bn is not None else NormPass(**dropout)


# ------------------------------------------------------------------------------------------------
# parameter layout
# ------------------------------------------------------------------------------------------------


class LayerSpec:
    """One conv layer of a network: state_dict key, torch weight shape [a, b, 4, 4], offsets into the flat buffer.
    norm: the layer is followed by a norm; norm_kind 'instance' (no parameters), 'instance_affine' (InstanceNorm2d(affine=True):
    state_dict prefix norm_key, weight / bias at g_off / be_off of the PARAMETER buffer, nothing else) or 'batch' (BatchNorm2d: the
    same two parameters, and running statistics at rm_off / rv_off of the network's BUFFER block, counter bn_idx of its counter
    tensor, batch statistics at bs_off of its scratch).
    sn: the weight is spectrally normalised (the layout of torch.nn.utils.spectral_norm: `key` is ...weight_orig and follows the bias
    in the state_dict; u / v / sigma at u_off / v_off / s_off of the network's spectral-norm block, assign_spectral)."""
    __slots__ = ('key', 'a', 'b', 'stride', 'transposed', 'p_off', 'bias_key', 'b_off', 'act', 'norm', 'dropout', 'norm_kind',
                 'norm_key', 'g_off', 'be_off', 'rm_off', 'rv_off', 'bn_idx', 'bs_off', 'sn', 'u_off', 'v_off', 's_off')

    def __init__(self, key, a, b, stride, transposed, act, norm, dropout=False, bias_key=None, norm_kind='instance', norm_key=None):
        self.key, self.a, self.b, self.stride, self.transposed = key, a, b, stride, transposed
        self.act, self.norm, self.dropout, self.bias_key = act, norm, dropout, bias_key
        self.norm_kind = norm_kind if norm else None
        self.norm_key = norm_key
        self.p_off = self.b_off = self.g_off = self.be_off = self.rm_off = self.rv_off = self.bn_idx = self.bs_off = -1
        self.sn, self.u_off, self.v_off, self.s_off = False, -1, -1, -1

    @property
    def bn(self):
        return self.norm_kind == 'batch'

    @property
    def in_affine(self):
        return self.norm_kind == 'instance_affine'

    @property
    def norm_params(self):
        """The norm has a per-channel weight and bias in the parameter buffer."""
        return self.norm_kind in ('batch', 'instance_affine')

    @property
    def cout(self):
        return self.b if self.transposed else self.a

    @property
    def cin(self):
        return self.a if self.transposed else self.b


def assign_offsets(layers):
    """Lay the packed blocks out back to back (16-byte aligned); returns the flat length in floats."""
    off = 0
    for l in layers:
        l.p_off = off
        off += 16 * l.a * l.b
        if l.bias_key is not None:
            l.b_off = off
            off += (l.cout + 3) // 4 * 4
        if l.norm_params:     # a norm's weight / bias: parameters like any other (Adam, all-reduce, capture see one buffer)
            l.g_off = off
            off += (l.cout + 3) // 4 * 4
            l.be_off = off
            off += (l.cout + 3) // 4 * 4
    return off


_IN_DEFAULTS = {'eps': 1e-5, 'momentum': 0.1, 'track_running_stats': False}


def norm_kind_of(norm_layer, who):
    """'instance' | 'instance_affine' | 'batch' | 'syncbatch' for a constructor's norm_layer argument; anything else raises
    NotImplementedError.  'instance_affine' is functools.partial(nn.InstanceNorm2d, affine=True): keywords only, the others at
    torch's defaults (affine=False or absent: 'instance').
    BatchNorm2d and SyncBatchNorm are taken with their defaults only (eps 1e-5, momentum 0.1, affine, tracked running statistics).
    'syncbatch' is 'batch' in every respect (layout, buffers, scratch, kernels) plus "synchronise the batch statistics across ranks
    while the data-parallel path is on" (layer_kind, BNRun.dist)."""
    if norm_layer is nn.InstanceNorm2d:
        return 'instance'
    if norm_layer is nn.BatchNorm2d:
        return 'batch'
    if norm_layer is nn.SyncBatchNorm:
        return 'syncbatch'
    if isinstance(norm_layer, functools.partial) and norm_layer.func is nn.InstanceNorm2d and not norm_layer.args:
        kw = dict(norm_layer.keywords)
        affine = kw.pop('affine', False)
        if isinstance(affine, bool) and all(k in _IN_DEFAULTS and type(v) is type(_IN_DEFAULTS[k]) and v == _IN_DEFAULTS[k]
                                            for k, v in kw.items()):
            return 'instance_affine' if affine else 'instance'
    raise NotImplementedError(f"{who} implements norm_layer=nn.InstanceNorm2d or nn.BatchNorm2d (with their defaults) only -- and "
                              f"functools.partial(nn.InstanceNorm2d, affine=True), InstanceNorm2d with a learnable scale and shift, "
                              f"and nn.SyncBatchNorm, BatchNorm2d with the global batch's statistics under data parallelism --, "
                              f"got {norm_layer!r}")


def layer_kind(norm_kind):
    """The LayerSpec.norm_kind of a network built with norm_kind: a SyncBatchNorm network's layers ARE BatchNorm layers."""
    return 'batch' if norm_kind == 'syncbatch' else norm_kind


def param_keys(layers):
    """state_dict keys of a network's parameters, in the reference's order."""
    keys = []
    for l in layers:
        # (torch's spectral_norm deletes `weight` and registers `weight_orig`: it then follows the bias)
        keys += [k for k in ((l.bias_key, l.key) if l.sn else (l.key, l.bias_key)) if k is not None]
        if l.norm_params:
            keys += [l.norm_key + '.weight', l.norm_key + '.bias']
    return keys


def assign_buffers(layers):
    """Lay out the BatchNorm running statistics (the network's BUFFER block, which Adam never sees), the counters and the batch
    statistics scratch (PG_BN_SLOTS slots of fp64 (mean, unbiased var) per channel).  Returns (floats, counters, scratch doubles)."""
    off = idx = soff = 0
    for l in layers:
        if not l.bn:
            continue
        C4 = (l.cout + 3) // 4 * 4
        l.rm_off, l.rv_off, l.bn_idx, l.bs_off = off, off + C4, idx, soff
        off += 2 * C4
        idx += 1
        soff += BN_SLOTS * l.cout * 2
    return off, idx, soff


BN_SLOTS = 3              # running-stat updates per step a network can collect: the discriminator's three passes (trainer.py:66,97,99)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def buffer_views(bufs, counters, layers):
    """{state_dict key: view} of the BatchNorm buffers (running_mean, running_var: [C] fp32; num_batches_tracked: 0-d int64)."""
    out = {}
    for l in layers:
        if l.bn:
            out[l.norm_key + '.running_mean'] = bufs.as_strided((l.cout,), (1,), l.rm_off)
            out[l.norm_key + '.running_var'] = bufs.as_strided((l.cout,), (1,), l.rv_off)
            out[l.norm_key + '.num_batches_tracked'] = counters.as_strided((), (), l.bn_idx)
    return out


def init_buffers_(bufs, counters, layers):
    """BatchNorm2d's initial state: running_mean 0, running_var 1, num_batches_tracked 0."""
    with torch.no_grad():
        bufs.zero_()
        counters.zero_()
        for l in layers:
            if l.bn:
                bufs[l.rv_off:l.rv_off + l.cout].fill_(1.0)


SN_EPS = 1e-12            # torch.nn.utils.spectral_norm's eps (the kernels' SN_EPS)


def assign_spectral(layers):
    """Lay out the spectral-norm block of a network (fp32, outside the parameter buffer like the BatchNorm buffers): per normalised
    layer u [cout] and v [cin * 16] in torch's order (weight_u / weight_v of the state_dict), then one sigma per layer.  Returns its
    length in floats (0 without such layers)."""
    off = 0
    sn = [l for l in layers if l.sn]
    for l in sn:
        l.u_off = off
        off += (l.a + 3) // 4 * 4
        l.v_off = off
        off += l.b * 16
    for l in sn:
        l.s_off = off
        off += 1
    return (off + 3) // 4 * 4


def spectral_views(bufs, layers):
    """{state_dict key: view} of the spectral-norm buffers (weight_u [cout], weight_v [cin * 16])."""
    out = {}
    for l in layers:
        if l.sn:
            stem = l.key[:-len('_orig')]
            out[stem + '_u'] = bufs.as_strided((l.a,), (1,), l.u_off)
            out[stem + '_v'] = bufs.as_strided((l.b * 16,), (1,), l.v_off)
    return out


def init_spectral_(bufs, layers, generator=None):
    """The initial u, v of torch.nn.utils.spectral_norm: normalised standard-normal draws from the CPU generator, u then v, layer by
    layer (after the weights: the wrap follows the module's construction)."""
    views = spectral_views(bufs, layers)
    with torch.no_grad():
        bufs.zero_()
        for key, view in views.items():
            draw = torch.empty(view.numel()).normal_(0, 1, generator=generator)
            view.copy_(torch.nn.functional.normalize(draw, dim=0, eps=SN_EPS))


def spectral_items(layers, flat, eff, bufs, iterate=False):
    """The pg_spectral_item list of a network's normalised layers: weights in `flat`, normalised weights at the same offsets of `eff`
    (which are also the offsets of the blocks in a flat gradient), u / v / sigma in `bufs`.  flat = None: shapes only."""
    sn = [l for l in layers if l.sn]
    items = (L.SpectralItem * len(sn))()
    for it, l in zip(items, sn):
        it.Cout, it.Cin, it.iterate, it.g_off = l.a, l.b, 1 if iterate else 0, l.p_off
        if flat is not None:
            it.W, it.w_hat = L.ptr(flat, l.p_off), L.ptr(eff, l.p_off)
            it.u, it.v, it.sigma = L.ptr(bufs, l.u_off), L.ptr(bufs, l.v_off), L.ptr(bufs, l.s_off)
    return items


def spectral_workspace(layers, device):
    """A workspace for spectral_fwd / spectral_bwd over `layers` (one per stream that runs them)."""
    items = spectral_items(layers, None, None, None)
    nbytes = L.load().pg_spectral_workspace_bytes(len(items), items)
    return torch.zeros(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def spectral_fwd(layers, flat, eff, bufs, ws, iterate):
    """eff <- flat with every normalised layer's weight block divided by its sigma, everything else copied.  iterate: one power
    iteration first, u and v in `bufs` updated (torch's training-mode forward); else sigma from the stored u, v (eval mode).  sigma is
    left in `bufs` as well.  Up to five launches on the current stream (pg_spectral_fwd), no host read."""
    items = spectral_items(layers, flat, eff, bufs, iterate)
    L.check(L.load().pg_spectral_fwd(len(items), items, flat.data_ptr(), eff.data_ptr(), flat.numel(), ws.data_ptr(),
                                     ws.numel() * ws.element_size(), _stream()), 'pg_spectral_fwd')


def spectral_bwd(layers, eff, bufs, ws, gflat):
    """The weight blocks of the flat gradient `gflat` from "w.r.t. the normalised weight" to "w.r.t. the stored weight", in place, with
    the normalised weights, u, v and sigma spectral_fwd left in `eff` / `bufs`.  Two launches on the current stream (pg_spectral_bwd)."""
    items = spectral_items(layers, eff, eff, bufs)       # (W itself is not read by the backward pair)
    L.check(L.load().pg_spectral_bwd(len(items), items, gflat.data_ptr(), gflat.numel(), ws.data_ptr(),
                                     ws.numel() * ws.element_size(), _stream()), 'pg_spectral_bwd')


def torch_views(flat, layers):
    """{state_dict key: strided view of `flat` with the reference's shape} (weights [a,b,4,4], biases [cout])."""
    out = {}
    for l in layers:
        ab = l.a * l.b
        if l.bias_key is not None and l.sn:       # (param_keys' order)
            out[l.bias_key] = flat.as_strided((l.cout,), (1,), l.b_off)
        out[l.key] = flat.as_strided((l.a, l.b, 4, 4), (l.b, 1, 4 * ab, ab), l.p_off)
        if l.bias_key is not None and not l.sn:
            out[l.bias_key] = flat.as_strided((l.cout,), (1,), l.b_off)
        if l.norm_params:
            out[l.norm_key + '.weight'] = flat.as_strided((l.cout,), (1,), l.g_off)
            out[l.norm_key + '.bias'] = flat.as_strided((l.cout,), (1,), l.be_off)
    return out


def default_init_(flat, layers, generator=None):
    """torch's default Conv2d / ConvTranspose2d init (the reference's ``weights_init`` is a no-op,
    trainer.py:327-343): kaiming_uniform_(a=sqrt(5)) = U(+-1/sqrt(fan_in)), fan_in = size(1)*16; bias
    U(+-1/sqrt(fan_in)).  Drawn in state_dict order with the CPU generator like nn.Module construction would."""
    views = torch_views(flat, layers)
    with torch.no_grad():
        for l in layers:
            bound = 1.0 / math.sqrt(l.b * 16)
            w = torch.empty(l.a, l.b, 4, 4).uniform_(-bound, bound, generator=generator)
            views[l.key].copy_(w)
            if l.bias_key is not None:
                bb = torch.empty(l.cout).uniform_(-bound, bound, generator=generator)
                views[l.bias_key].copy_(bb)
            if l.norm_params:     # reset_parameters of BatchNorm2d / affine InstanceNorm2d: weight 1, bias 0 (draws nothing from the generator)
                views[l.norm_key + '.weight'].fill_(1.0)
                views[l.norm_key + '.bias'].zero_()


# ------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------


def unet_layers(input_nc, output_nc, nf, activation, final_act, use_dropout, norm_kind='instance'):
    """Layer plan of reference UNet.__init__ (unet.py:84-107).  norm_kind 'batch' / 'instance_affine': norm blocks with parameters
    (DownNorm{i} / UpNorm{i})."""
    if activation not in ('tanh', 'relu', 'leakyrelu'):
        raise ValueError(f"activation must be one of tanh|relu|leakyrelu, got {activation!r}")
    if final_act not in ('tanh', 'relu', 'leakyrelu', 'sigmoid', 'softmax'):
        raise ValueError(f"final_act must be one of tanh|relu|leakyrelu|sigmoid|softmax, got {final_act!r}")
    filts = [nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8]
    enc, dec = [], []
    prev = input_nc
    for i, f in enumerate(filts):
        enc.append(LayerSpec(f'encoder.{i}.model.DownConv{i}.weight', f, prev, 2, False, activation, True, use_dropout,
                             norm_kind=norm_kind, norm_key=f'encoder.{i}.model.DownNorm{i}'))
        prev = f
    for i, f in enumerate(filts[:-1][::-1]):
        cin = prev if i == 0 else prev * 2
        dec.append(LayerSpec(f'decoder.{i}.model.UpConv{i}.weight', cin, f, 2, True, activation, i != 0,
                             use_dropout and i != 0, norm_kind=norm_kind, norm_key=f'decoder.{i}.model.UpNorm{i}'))
        prev = f
    dec.append(LayerSpec('decoder.6.model.UpConv6.weight', nf * 2, output_nc, 2, True, final_act, False, False))
    return enc, dec


class GenContext:
    """Activations saved by one generator forward (what autograd would have kept)."""
    pass


class _WeightPrep:
    """Per-step weight preparation of a network (mixed into the two engines).  ucache_begin() opens the cache for one weight version:
    from the second step of a given kind on it comes back already filled by one batched launch (prefill_ucache) with what the previous
    such step used; ucache_end() remembers what this step used.

    Memory: the transformed / packed weights depend on the layer, the direction and the transform (all three are in the entry key,
    which carries the byte count), NOT on the input extent -- so the device buffers live in ONE pool per network keyed by entry,
    shared by every extent and mode (a ragged last batch or a second image size adds no device memory).  The per-(extent, mode)
    fill plans are small host lists, kept for the MAX_PLANS most recently used kinds of step.  clear_weight_caches() (called by
    set_precision / set_tuning) drops both."""

    MAX_PLANS = 8

    def _init_network(self, layers, norm_kind, algo):
        """The constructor tail of both engines: parameter / buffer layout of `layers`, norm kind (norm_kind_of's), algorithm, caches."""
        self.layers, self.norm_kind = layers, norm_kind
        self.nparams = assign_offsets(layers)
        self.has_bn = any(l.bn for l in layers)
        self.sync_bn = self.has_bn and norm_kind == 'syncbatch'
        self.nbuf, self.nbn, self.nscratch = assign_buffers(layers)
        self.spectral, self.nsn = False, 0      # (spectral normalisation: the discriminator's option, DiscriminatorEngine)
        self.algo = DEFAULT_ALGO if algo is None else algo
        self.act_bf = False          # bf16 activation storage (set_precision('bf16'); only where bf16_storage_ok())
        self._ops = {}
        self._sok = {}

    def _storage_ok(self, key, interior_ops):
        if key not in self._sok:
            self._sok[key] = _bf16_tensors_ok(interior_ops, self._LD_MULT)
        return self._sok[key]

    def ucache_begin(self, flat, N, H, W, tag=None):
        key = (N, H, W, tag, self.algo, bool(self.act_bf))
        pool = self.__dict__.setdefault('_upool', {})
        plans = self.__dict__.setdefault('_uplan', {})
        plan = plans.pop(key, None)
        if plan is not None:
            plans[key] = plan          # most recently used last
        uc = prefill_ucache(plan, flat, flat.device, pool)
        uc.plan_key = key
        return uc

    def ucache_end(self, uc):
        if isinstance(uc, UCache) and getattr(uc, 'plan_key', None) is not None:
            plans = self.__dict__.setdefault('_uplan', {})
            plans.pop(uc.plan_key, None)
            plans[uc.plan_key] = list(uc.log)
            while len(plans) > self.MAX_PLANS:
                plans.pop(next(iter(plans)))
            # buffers no remembered plan refers to any more (entries of evicted plans) go back to the allocator
            pool = self.__dict__.get('_upool', {})
            live = {e[0] for p in plans.values() for e in p} | set(uc.keys())
            for k in [k for k in pool if k not in live]:
                del pool[k]

    def clear_weight_caches(self):
        self.__dict__.pop('_upool', None)
        self.__dict__.pop('_uplan', None)


class GeneratorEngine(_WeightPrep):
    _LD_MULT = 2          # interior tensors are channel slices of the skip-connection buffers cat_i (twice their channels)

    def __init__(self, input_nc, output_nc, nf, activation, final_act, use_dropout, algo=None, norm_kind='instance'):
        self.input_nc, self.output_nc, self.nf = input_nc, output_nc, nf
        self.activation, self.final_act, self.use_dropout = activation, final_act, use_dropout
        self.enc, self.dec = unet_layers(input_nc, output_nc, nf, activation, final_act, use_dropout, layer_kind(norm_kind))
        self._init_network(self.enc + self.dec, norm_kind, algo)

    def bf16_storage_ok(self):
        """Every interior tensor feeds / comes from a fast bf16 conv kernel: channel counts multiples of 4 and >= 32."""
        return self.nf % 4 == 0 and self.nf >= 32

    def ops(self, N, H, W):
        """ConvOps for input extent (N, H, W); cached."""
        key = (N, H, W)
        if key not in self._ops:
            enc_ops, dec_ops = [], []
            h, w = H, W
            for l in self.enc:
                op = ConvOp(N, h, w, l.a, l.b, 2, self.algo)
                enc_ops.append(op)
                h, w = op.Hs, op.Ws
                if h * w <= 1 and not self.has_bn:     # torch raises from this block's InstanceNorm before the next conv is reached
                    # (BatchNorm needs N*H*W > 1 in training mode only: batchnorm_act_fwd checks it per pass)
                    raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                                     f"torch.Size([{N}, {l.a}, {h}, {w}])")
            sizes = [(op.Hs, op.Ws) for op in enc_ops]   # enc i output extent
            for i, l in enumerate(self.dec):
                # convT: small = input (h, w), big = output (2h, 2w)
                op = ConvOp(N, 2 * h, 2 * w, l.a, l.b, 2, self.algo)
                assert (op.Hs, op.Ws) == (h, w)
                dec_ops.append(op)
                h, w = 2 * h, 2 * w
                if i < 6:
                    sh, sw = sizes[5 - i]
                    if (sh, sw) != (h, w):
                        raise RuntimeError(f"Sizes of tensors must match except in dimension 1. Expected size {h} but got "
                                           f"size {sh} for the skip connection of decoder block {i + 1} (input {H}x{W}: "
                                           "H and W must be multiples of 128)")
            self._ops[key] = (enc_ops, dec_ops)
        return self._ops[key]

    def forward(self, flat, xin, gen_out, train, seed=0, sample0=0, keep_v=False, ucache=None, bn=None):
        """xin: View [N,H,W,input_nc]; gen_out: View [N,H,W,output_nc] to receive final_act(dec6).
        train selects dropout (InstanceNorm always uses instance statistics, unet.py:77).  sample0 = index of this
        batch's first sample in the global batch (data parallelism: the dropout masks are those of the global batch).
        keep_v: a backward pass follows -- encoder layers on the polyphase Winograd path keep their transformed input for the
        weight gradient (pg_conv_extras.v_keep / v_pre) instead of transforming it again.
        ucache: a dict the caller keeps for as long as `flat` is unchanged (Trainer.batch: forward + backward of one step): on bf16
        tensors a layer's packed bf16 weights are built once and serve both its forward and its data gradient.
        bn: a BNRun (BatchNorm networks only)."""
        assert bn is not None or not self.has_bn, 'a BatchNorm generator pass needs its BNRun'
        N, H, W = xin.N, xin.H, xin.W
        dev = flat.device
        enc_ops, dec_ops = self.ops(N, H, W)
        F = [l.a for l in self.enc]
        c = GenContext()
        c.N, c.H, c.W, c.xin, c.gen_out = N, H, W, xin, gen_out
        norm = c.norm = norm_pass(bn, train=train, seed=seed, sample0=sample0)
        # cat_i (i = 1..6): input of decoder i = [dec_{i-1} out | enc_{6-i} out]
        # bf16 activation storage: every interior activation (conv outputs, normalised outputs, their gradients) is a bf16 tensor;
        # the image-facing tensors (x, enc0's conv output, the generator output and its gradient) stay fp32 and the InstanceNorm /
        # activation kernels next to them read one type and write the other
        bf = c.bf = bool(self.act_bf) and self._storage_ok((N, H, W), enc_ops[1:] + dec_ops[:6])
        # ... unless they fit 8-channel pixels: then x and dL/d(output) are padded to that bf16 layout (one small pass each) and the
        # first / last layer run on the bf16 kernels as well (SEAM8)
        # (nf % 64: the row GEMMs next to the images -- the head's forward over 2 * nf channels, the data gradient onto x over nf --
        # contract in 64-wide chunks)
        seam8 = c.seam8 = (bf and SEAM8 and self.nf % 64 == 0 and self.input_nc <= 8 and self.output_nc <= 8
                           and enc_ops[0].describe(0, L.IO_MASK)[0].startswith('k_conv_bf16x'))      # (not with PG_TUNE_BF16X_OFF)
        c.xin8 = xin.padded8() if seam8 else None
        c.cat = [None] * 7
        for i in range(1, 7):
            op = dec_ops[i]
            c.cat[i] = View.alloc(N, op.Hs, op.Ws, self.dec[i].a, dev, bf=bf)
        c.hidden = View.alloc(N, enc_ops[6].Hs, enc_ops[6].Ws, F[6], dev, bf=bf)
        c.y, c.stats, c.enc_out, c.v = [], [], [], []
        act = L.ACT_CODES[self.activation]
        src = c.xin8 if seam8 else xin
        for i, (l, op) in enumerate(zip(self.enc, enc_ops)):
            y = View.alloc(N, op.Hs, op.Ws, l.a, dev, bf=bf and (i > 0 or seam8))
            if i < 6:
                cat = c.cat[6 - i]
                out = cat.channels(cat.C - l.a, l.a)
            else:
                out = c.hidden
            vk = op.keep_v(keep_v, src, y)
            u, uv = _ucache(ucache, ('e', i), 0, op, dev, src, y, l.p_off)
            c.stats.append(norm.conv_norm_act(op, 0, src, flat, l, (1, i), y, out, act, v_keep=vk, u_cache=u, u_valid=uv))
            c.v.append(vk)
            c.y.append(y)
            c.enc_out.append(out)
            src = out
        c.yd, c.statsd = [None] * 7, [None] * 7
        src = c.hidden
        for i, (l, op) in enumerate(zip(self.dec, dec_ops)):
            if i == 6:
                # the 1..4-channel head: taps folded into N (row GEMM + col2im); fp32 kernels on an fp32 copy of its input, or the
                # bf16 row GEMM straight from the bf16 tensor
                src = c.cat6_f32 = src if seam8 else src.converted(False)
                if self.final_act == 'softmax':
                    c.gen_raw = View.alloc(N, op.Hb, op.Wb, l.b, dev)
                    op.small2big(src, flat, l.p_off, None, 0, c.gen_raw)
                    softmax_fwd(c.gen_raw, gen_out)
                else:
                    op.small2big(src, flat, l.p_off, None, 0, gen_out, L.ACT_CODES[self.final_act])
                break
            cat = c.cat[i + 1]
            out = cat.channels(0, l.b)
            if l.norm:
                yd = View.alloc(N, op.Hb, op.Wb, l.b, dev, bf=bf)
                u, uv = _ucache(ucache, ('d', i), 1, op, dev, src, yd, l.p_off)
                c.yd[i], c.statsd[i] = yd, norm.conv_norm_act(op, 1, src, flat, l, (2, i), yd, out, act, u_cache=u, u_valid=uv)
            else:
                op.small2big(src, flat, l.p_off, None, 0, out, act)
            src = cat
        return c

    def backward(self, flat, gflat, c, g1, g2=None, need_dx=False, on_ready=None, ucache=None, defer_join=False):
        """g1 (+ g2): Views of dL/d(gen_out).  Writes every weight gradient into `gflat` (packed layout);
        returns dL/dx as a View if need_dx.  on_ready(lo, hi) is called after each layer's weight gradient has been
        enqueued with that layer's range of the flat buffer (last layer first): the hook data parallelism uses to
        start all-reducing finished buckets under the rest of the backward pass."""
        def done(l):
            if on_ready is not None:
                # (a norm's weight / bias gradients follow its conv block in the flat buffer and are written before it)
                on_ready(l.p_off, l.be_off + (l.cout + 3) // 4 * 4 if l.norm_params else l.p_off + 16 * l.a * l.b)
        # defer_join: the caller joins the second stream itself (side_join()) before it reads the weight gradients -- the trainer puts
        # the discriminator's forward pass, which needs none of them, in between
        _side_begin(not self.act_bf or BF16_WGRAD_SIDE)       # (bf16: the two chains contend for the L1 path: 5.87 -> 5.94 ms at cfg4)
        ok = False
        try:
            r = self._backward(flat, gflat, c, g1, g2, need_dx, done, ucache)
            ok = True
            return r
        finally:
            if not (ok and defer_join):
                _side_join()
            else:
                cur_exec().allow = False

    def _backward(self, flat, gflat, c, g1, g2, need_dx, done, ucache):
        N, dev = c.N, flat.device
        enc_ops, dec_ops = self.ops(c.N, c.H, c.W)
        act = L.ACT_CODES[self.activation]
        # ---- decoder, last to first
        l, op = self.dec[6], dec_ops[6]
        dy = View.alloc(N, op.Hb, op.Wb, l.b, dev)
        if self.final_act == 'softmax':
            softmax_bwd(g1, g2, c.gen_out, dy)
        else:
            act_bwd(g1, g2, c.gen_out, dy, L.ACT_CODES[self.final_act])
        bf = c.bf
        if c.seam8:
            dy = dy.padded8()
        dcat = View.alloc(N, op.Hs, op.Ws, l.a, dev, bf=c.seam8)  # fp32 with the head's fp32 kernels; the blocks below read it as is
        op.bwd_big(c.cat6_f32, dy, flat, gflat, l.p_off, dcat)    # weight gradient + data gradient of the ConvTranspose2d
        done(l)
        dskip = [None] * 7   # dskip[j]: gradient wrt enc_j output arriving through the skip connection
        for i in range(5, -1, -1):
            l, op = self.dec[i], dec_ops[i]
            g = dcat.channels(0, l.b)
            dskip[5 - i] = dcat.channels(l.b, dcat.C - l.b)
            dy = View.alloc(N, op.Hb, op.Wb, l.b, dev, bf=bf)
            if l.norm:
                c.norm.backward(l, gflat, g, None, c.yd[i], c.statsd[i], dy, act, key=(2, i))
            else:
                act_bwd(g, None, c.cat[i + 1].channels(0, l.b), dy, act)
            src = c.hidden if i == 0 else c.cat[i]
            dsrc = View.alloc(N, op.Hs, op.Ws, l.a, dev, bf=bf)
            u, uv = _ucache(ucache, ('d', i), 0, op, dev, dy, dsrc, l.p_off)
            if (u is not None and bf) or (SPLIT_BWD_BIG and cur_exec().allow):      # bf16 tensors: the two halves as two calls, the data gradient on the forward's packed weights
                vk = op.keep_v(SHARE_DY_V and not bf, dy, dsrc, src)
                if vk is not None:
                    # both halves start from the polyphase transform of dy: the data gradient keeps it (v_keep), the weight gradient --
                    # on the second stream, behind this layer's data gradient instead of beside it -- takes it over (v_pre)
                    op.big2small(dy, flat, l.p_off, None, 0, dsrc, u_cache=u, u_valid=uv, v_keep=vk)
                    op.wgrad(src, dy, gflat, l.p_off, v_pre=vk)
                else:
                    op.wgrad(src, dy, gflat, l.p_off)
                    op.big2small(dy, flat, l.p_off, None, 0, dsrc, u_cache=u, u_valid=uv)
            else:
                op.bwd_big(src, dy, flat, gflat, l.p_off, dsrc, u_cache=u, u_valid=uv)
            done(l)
            dcat = dsrc
        # ---- encoder, last to first; dcat is now dL/d(hidden)
        g_main = dcat
        dx = None
        for j in range(6, -1, -1):
            l, op = self.enc[j], enc_ops[j]
            dy = View.alloc(N, op.Hs, op.Ws, l.a, dev, bf=bf and (j > 0 or c.seam8))
            c.norm.backward(l, gflat, g_main, dskip[j] if j < 6 else None, c.y[j], c.stats[j], dy, act, key=(1, j))
            src = (c.xin8 if c.seam8 else c.xin) if j == 0 else c.enc_out[j - 1]
            op.wgrad(dy, src, gflat, l.p_off, v_pre=c.v[j] if ConvOp._aligned(dy, src) else None)
            done(l)
            if j > 0 or need_dx:
                dsrc = View.alloc(N, op.Hb, op.Wb, l.b, dev, bf=bf and j > 0)
                u, uv = _ucache(ucache, ('e', j), 1, op, dev, dy, dsrc, l.p_off)
                op.small2big(dy, flat, l.p_off, None, 0, dsrc, u_cache=u, u_valid=uv)
                if j == 0:
                    dx = dsrc
                g_main = dsrc
        return dx


# ------------------------------------------------------------------------------------------------
# discriminator
# ------------------------------------------------------------------------------------------------


DISC_FINAL_ACTS = ('sigmoid', 'none')


def disc_layers(input_nc, ndf, n_layers, norm, norm_kind='instance', spectral=False, final_act='sigmoid'):
    """Layer plan of reference Discriminator.__init__ (disc.py:19-46); keys are nn.Sequential indices (a norm is the third module
    of its block: Conv, Tanh, norm).  spectral: every conv as torch.nn.utils.spectral_norm leaves it (weight -> weight_orig).
    final_act: 'sigmoid' (the reference's nn.Sigmoid behind the head conv) or 'none' (the head's logits; nn.Sigmoid has no state, so
    keys, offsets and the flat buffer are the same)."""
    if final_act not in DISC_FINAL_ACTS:
        raise ValueError(f"final_act must be one of {' | '.join(DISC_FINAL_ACTS)}, got {final_act!r}")
    layers = []
    idx = 0
    layers.append(LayerSpec(f'model.{idx}.weight', ndf, input_nc, 2, False, 'leakyrelu', False, bias_key=f'model.{idx}.bias'))
    idx += 2
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        layers.append(LayerSpec(f'model.{idx}.weight', ndf * mult, ndf * prev, 2, False, 'tanh', norm, norm_kind=norm_kind,
                                norm_key=f'model.{idx + 2}'))
        idx += 3 if norm else 2
    prev, mult = mult, min(2 ** n_layers, 8)
    layers.append(LayerSpec(f'model.{idx}.weight', ndf * mult, ndf * prev, 1, False, 'tanh', norm, norm_kind=norm_kind,
                            norm_key=f'model.{idx + 2}'))
    idx += 3 if norm else 2
    layers.append(LayerSpec(f'model.{idx}.weight', 1, ndf * mult, 1, False, final_act, False, bias_key=f'model.{idx}.bias'))
    if spectral:
        for l in layers:
            l.key, l.sn = l.key + '_orig', True
    return layers


class DiscContext:
    def samples(self, n0, n):
        """The context of samples [n0, n0 + n) of this pass, for a backward pass WITHOUT weight gradients (the generator step's data
        gradient through D reads the fake half of the step's one 2N context): views of the same tensors, no kept V."""
        assert not self.bf and not any(s is not None for s in self.stats), 'sample views: fp32 contexts without a norm layer'
        c = DiscContext()
        c.N, c.H, c.W = n, self.H, self.W
        c.norm, c.bf, c.seam8 = self.norm, self.bf, self.seam8
        c.din = self.din.samples(n0, n)
        c.t, c.a, c.src = ([v.samples(n0, n) for v in vs] for vs in (self.t, self.a, self.src))
        c.stats, c.v = list(self.stats), [None] * len(self.v)
        c.out = c.a[-1]
        return c


class DiscriminatorEngine(_WeightPrep):
    _LD_MULT = 1

    def __init__(self, input_nc, ndf, n_layers, norm, algo=None, norm_kind='instance', spectral=False, final_act='sigmoid'):
        self.input_nc, self.ndf, self.n_layers, self.norm = input_nc, ndf, n_layers, norm
        self._init_network(disc_layers(input_nc, ndf, n_layers, norm, layer_kind(norm_kind), spectral, final_act), norm_kind, algo)
        self.final_act = final_act
        self.spectral = bool(spectral)
        self.nsn = assign_spectral(self.layers)
        if self.spectral and len(self.layers) > L.SN_MAX_LAYERS:
            raise NotImplementedError(f"patchgan_amd: spectral_norm takes at most {L.SN_MAX_LAYERS} conv layers (n_layers <= "
                                      f"{L.SN_MAX_LAYERS - 2}), got n_layers = {n_layers}")

    def bf16_storage_ok(self):
        return self.ndf % 4 == 0 and self.ndf >= 32

    def ops(self, N, H, W):
        key = (N, H, W)
        if key not in self._ops:
            ops = []
            h, w = H, W
            for l in self.layers:
                op = ConvOp(N, h, w, l.a, l.b, l.stride, self.algo)
                ops.append(op)
                h, w = op.Hs, op.Ws
            self._ops[key] = ops
        return self._ops[key]

    def out_shape(self, N, H, W):
        op = self.ops(N, H, W)[-1]
        return (N, 1, op.Hs, op.Ws)

    def halves_ok(self, N, H, W):
        """One pass over 2 N samples may be run as two passes over N samples each that fill one context (forward_part): a network
        without norm layers on fp32 tensors, every layer's N-sample call doing per sample what its 2 N-sample call does
        (ConvOp.halves_same), and every layer's second half starting on a 16-byte boundary (the views of the two halves then take
        the same kernels as the whole tensor's).  InstanceNorm / BatchNorm discriminators and bf16 networks answer False: their
        callers keep the separate passes."""
        key = ('halves', N, H, W)
        if key not in self._ops:
            ok = not self.norm and not self.act_bf and (self.algo & L.ALGO_MASK) in (L.ALGO_AUTO, L.ALGO_MFMA, L.ALGO_DIRECT)
            if ok:
                half, whole = self.ops(N, H, W), self.ops(2 * N, H, W)
                ok = all(h.halves_same(w) and (N * h.Hs * h.Ws * h.Ca * 4) % 16 == 0 for h, w in zip(half, whole))
            self._ops[key] = ok
        return self._ops[key]

    def context(self, flat, din, keep_v=False):
        """An empty context of a pass over din [Nt,H,W,input_nc] (needs halves_ok(Nt / 2, H, W)): every layer's output tensor and
        kept transform allocated for Nt samples, nothing launched.  forward_part() fills it half by half; once both halves are in
        it is what forward(flat, din, keep_v=keep_v) returns."""
        ops = self.ops(din.N, din.H, din.W)
        dev = flat.device
        c = DiscContext()
        c.din, c.N, c.H, c.W = din, din.N, din.H, din.W
        c.norm, c.bf, c.seam8 = norm_pass(None), False, False
        c.t, c.stats, c.a, c.v, c.src = [], [], [], [], []
        src = din
        for l, op in zip(self.layers, ops):
            c.src.append(src)
            t = View.alloc(din.N, op.Hs, op.Ws, l.a, dev)
            c.v.append(op.keep_v(keep_v, src, t))
            c.t.append(t)
            c.stats.append(None)
            c.a.append(t)
            src = t
        c.out = src
        return c

    def forward_part(self, flat, c, n0, n, ucache=None):
        """Samples [n0, n0 + n) of the pass whose context c is (context()): the n-sample plan of every layer, reading and writing
        the sample ranges of c's tensors; a kept transform goes into its rows of the whole batch's buffer (ConvOp.v_part)."""
        whole = self.ops(c.N, c.H, c.W)
        dev = flat.device
        for li, (l, op) in enumerate(zip(self.layers, self.ops(n, c.H, c.W))):
            src, t = c.src[li].samples(n0, n), c.t[li].samples(n0, n)
            bias = flat if l.bias_key is not None else None
            u, uv = _ucache(ucache, li, 0, op, dev, src, t, l.p_off)
            vk = c.v[li]
            op.big2small(src, flat, l.p_off, bias, l.b_off, t, L.ACT_CODES[l.act], v_keep=vk, u_cache=u, u_valid=uv,
                         v_part=op.v_part(whole[li], n0) if vk is not None else (0, 0))

    def forward(self, flat, din, ucache=None, keep_v=False, bn=None):
        """din: View [N,H,W,input_nc].  Returns a context; ctx.out is the patch map View [N,h,w,1] (probabilities, or logits with final_act='none').
        ucache: a dict owned by the caller that lives exactly as long as the weights in `flat` stay unchanged (Trainer.batch: one
        step) -- the Winograd-transformed weights are computed once per (layer, direction) and reused by every pass that
        shares the dict.  keep_v: a backward pass with weight gradients follows (see GeneratorEngine.forward).  bn: a BNRun (BatchNorm
        networks only)."""
        assert bn is not None or not self.has_bn, 'a BatchNorm discriminator pass needs its BNRun'
        ops = self.ops(din.N, din.H, din.W)
        dev = flat.device
        c = DiscContext()
        c.din, c.N, c.H, c.W = din, din.N, din.H, din.W
        norm = c.norm = norm_pass(bn)
        c.t, c.stats, c.a, c.v, c.src = [], [], [], [], []
        # bf16 activation storage: the tensors between the first and the last layer are bf16; the input (x | mask), the first
        # layer's conv output (4-channel input: generic kernel) and the 1-channel head stay fp32
        last = len(self.layers) - 1
        bf = c.bf = bool(self.act_bf) and self._storage_ok((din.N, din.H, din.W), ops[1:last])
        # the input in 8-channel bf16 pixels where it fits: the first layer then runs on the bf16 kernels too (GeneratorEngine.forward)
        # (ndf % 64: the data gradient onto x | mask is a row GEMM contracting over ndf channels in 64-wide chunks)
        seam8 = c.seam8 = (bf and SEAM8 and self.ndf % 64 == 0 and self.input_nc <= 8 and last > 0
                           and ops[0].describe(0, L.IO_MASK)[0].startswith('k_conv_bf16x'))

        src = din.padded8() if seam8 else din
        for li, (l, op) in enumerate(zip(self.layers, ops)):
            if li == last:
                src = src.converted(False)
            c.src.append(src)
            t = View.alloc(din.N, op.Hs, op.Ws, l.a, dev, bf=bf and (0 < li < last or (li == 0 and seam8)))
            bias = flat if l.bias_key is not None else None
            u, uv = _ucache(ucache, li, 0, op, dev, src, t, l.p_off)
            vk = op.keep_v(keep_v, src, t)
            c.v.append(vk)
            op.big2small(src, flat, l.p_off, bias, l.b_off, t, L.ACT_CODES[l.act], v_keep=vk, u_cache=u, u_valid=uv)   # conv + bias + act fused
            if l.norm:                                                              # disc.py:31-32: Conv -> Tanh -> norm
                a = View.alloc(din.N, op.Hs, op.Ws, l.a, dev, bf=bf and li < last)
                stats = norm.norm_act(l, flat, t, a, L.ACT_NONE)
            else:
                if bf and li == 0 and not seam8:
                    t = t.converted(True)          # the next layer's kernel reads bf16
                a, stats = t, None
            c.t.append(t)
            c.stats.append(stats)
            c.a.append(a)
            src = a
        c.out = src
        return c

    def backward(self, flat, gflat, c, gout, need_wgrad=True, need_dx=False, ucache=None):
        """gout: View of dL/d(out).  need_wgrad=False skips the weight gradients (the generator step's pass
        through D, whose D-gradients the reference zeroes at trainer.py:93-94).  ucache: as in forward."""
        _side_begin(need_wgrad and (not self.act_bf or BF16_WGRAD_SIDE))
        try:
            return self._backward(flat, gflat, c, gout, need_wgrad, need_dx, ucache)
        finally:
            _side_join()

    def _backward(self, flat, gflat, c, gout, need_wgrad, need_dx, ucache):
        ops = self.ops(c.N, c.H, c.W)
        dev = flat.device
        g = gout
        dx = None
        bf, last = c.bf, len(self.layers) - 1
        inner_of = lambda i: bf and (0 < i < last or (i == 0 and c.seam8))
        fused = None        # dy of this layer, already produced by the data-gradient kernel of the layer above
        for li in range(last, -1, -1):
            l, op = self.layers[li], ops[li]
            inner = inner_of(li)
            if fused is not None:
                dy, fused = fused, None
            else:
                if l.norm:
                    dt = View.alloc(c.N, op.Hs, op.Ws, l.a, dev, bf=inner)
                    c.norm.backward(l, gflat if need_wgrad else None, g, None, c.t[li], c.stats[li], dt, L.ACT_NONE)
                    g = dt
                if li == last and not l.norm and L.ACT_CODES[l.act] == L.ACT_NONE:
                    dy = g          # a logit head: its activation backward is the identity -- no launch, gout is the head's dy
                else:
                    dy = View.alloc(c.N, op.Hs, op.Ws, l.a, dev, bf=inner)
                    act_bwd(g, None, c.t[li], dy, L.ACT_CODES[l.act])
            src = c.src[li]
            if need_wgrad:
                op.wgrad(dy, src, gflat, l.p_off, gflat if l.bias_key is not None else None, l.b_off,
                         v_pre=c.v[li] if ConvOp._aligned(dy, src) else None)
            if li > 0 or need_dx:
                # the activation backward of the layer below (no InstanceNorm in between) in this kernel's epilogue: the tensor it
                # writes is then that layer's dy (and has dy's storage type)
                below = self.layers[li - 1] if li > 0 else None
                dsrc = None
                if FUSE_ACT_BWD and below is not None and not below.norm:
                    cand = View.alloc(c.N, op.Hb, op.Wb, l.b, dev, bf=inner_of(li - 1))
                    if op.mul_ok(dy, cand, c.t[li - 1]):
                        dsrc = fused = cand
                if dsrc is None:
                    dsrc = View.alloc(c.N, op.Hb, op.Wb, l.b, dev, bf=bf and 0 < li < last)
                u, uv = _ucache(ucache, li, 1, op, dev, dy, dsrc, l.p_off)
                if fused is not None:
                    op.small2big(dy, flat, l.p_off, None, 0, dsrc, u_cache=u, u_valid=uv, mul=(c.t[li - 1], L.ACT_CODES[below.act]))
                else:
                    op.small2big(dy, flat, l.p_off, None, 0, dsrc, u_cache=u, u_valid=uv)
                g = dsrc
                if li == 0:
                    dx = dsrc
        return dx


# ------------------------------------------------------------------------------------------------
# losses on the device
# ------------------------------------------------------------------------------------------------


class LossBuffers:
    """Scratch for one loss evaluation: S f64 (the per-(sample, channel) reduction terms: COMBINED [N*C*5] sums on the staged path,
    the nsplit partial slabs on the one-launch path, which combines them inside pg_loss_value_grad), sums [2] f64, coef [N*C*2] f32.
    Kept alive by the caller until the launches that use it are enqueued; nothing reads it afterwards."""

    def __init__(self, N, C, device, HW=1):
        self.S = torch.empty(int(L.load().pg_loss_reduce_doubles(N, HW, C)), dtype=torch.float64, device=device)
        self.sums = torch.empty(2, dtype=torch.float64, device=device)      # (written by pg_loss_prepare where it is read at all)
        self.coef = torch.empty(N * C * 2, dtype=torch.float32, device=device)


class PendingLoss:
    """A loss evaluation whose batch-global reduction terms are still being summed across ranks."""
    __slots__ = ('buf', 'wait', 'args', 'nsplit', 'sums')


def _fused_loss_max_nc():
    """pg_loss_value_grad's table (N * C entries) lives in LDS: the library says how many fit (pg_loss_fused_max_nc)."""
    global _FUSED_LOSS_MAX_NC
    if _FUSED_LOSS_MAX_NC is None:
        _FUSED_LOSS_MAX_NC = int(L.load().pg_loss_fused_max_nc())
    return _FUSED_LOSS_MAX_NC


_FUSED_LOSS_MAX_NC = None


def loss_begin(p, y, tconst, beta=0.75, allreduce=None, need_sums=True):
    """Phase 1 of a loss term over prediction View p against target View y (or the constant tconst): the per-sample
    reductions and the two batch-global terms.  `allreduce(tensor)` starts their SUM across ranks under data parallelism
    and returns a wait() callable; anything enqueued between loss_begin and loss_finish overlaps that exchange.
    In one process there is nothing to exchange between the phases: phase 1 is then ONE launch (pg_loss_reduce_parts) and phase 2
    one more (pg_loss_value_grad adds the partial slabs, forms the batch-global terms, the value and the gradient)."""
    lib = L.load()
    buf = LossBuffers(p.N, p.C, p.t.device, p.HW)
    st = _stream()
    h = PendingLoss()
    h.buf, h.args, h.wait, h.sums = buf, (p, y, tconst, beta), None, None
    yp, yl = _pl(y)
    exchange = allreduce is not None and need_sums
    if not exchange and p.N * p.C <= _fused_loss_max_nc():
        h.nsplit = int(lib.pg_loss_reduce_parts(p.ptr(), p.ld, yp, yl, float(tconst), p.N, p.HW, p.C, buf.S.data_ptr(), st))
        if h.nsplit < 1:
            L.check(h.nsplit, 'pg_loss_reduce_parts')
        return h
    h.nsplit = 0          # staged: S is the combined result
    L.check(lib.pg_loss_reduce(p.ptr(), p.ld, yp, yl, float(tconst), p.N, p.HW, p.C, buf.S.data_ptr(), st), 'pg_loss_reduce')
    if need_sums:      # the two batch-global terms: only focal-Tversky and weighted BCE read them
        L.check(lib.pg_loss_prepare(buf.S.data_ptr(), p.N, p.C, beta, buf.sums.data_ptr(), st), 'pg_loss_prepare')
        h.sums = buf.sums
    if exchange:
        h.wait = allreduce(buf.sums)
    return h


def loss_finish(h, mode, alpha, grad_out, loss_out, loss_slot, bglobal, gamma=0.75):
    """Phase 2: the loss value into loss_out[loss_slot] and, if grad_out is not None, its gradient wrt p into View
    grad_out (seeded with the GLOBAL batch terms).  Returns the scratch buffers (see LossBuffers: not a result)."""
    lib = L.load()
    p, y, tconst, beta = h.args
    buf = h.buf
    if h.wait is not None:
        h.wait()
    st = _stream()
    yp, yl = _pl(y)
    sums = h.sums.data_ptr() if h.sums is not None else None
    if p.N * p.C <= _fused_loss_max_nc():
        gp, gl = _pl(grad_out)
        L.check(lib.pg_loss_value_grad(buf.S.data_ptr(), max(h.nsplit, 1), None, sums, mode, p.N, p.C, p.HW, bglobal, alpha, beta, gamma,
                                       p.ptr(), p.ld, yp, yl, float(tconst), gp, gl, L.ptr(loss_out, loss_slot), st), 'pg_loss_value_grad')
        return buf
    L.check(lib.pg_loss_finalize(buf.S.data_ptr(), sums, mode, p.N, p.C, p.HW, bglobal, alpha, beta, gamma,
                                 buf.coef.data_ptr(), L.ptr(loss_out, loss_slot), st), 'pg_loss_finalize')
    if grad_out is not None:
        gmode = {L.LOSS_TVERSKY: 0, L.LOSS_WBCE: 1, L.LOSS_BCE: 1, L.LOSS_MAE: 2}[mode]
        L.check(lib.pg_loss_grad(p.ptr(), p.ld, yp, yl, float(tconst), buf.coef.data_ptr(), grad_out.ptr(), grad_out.ld, p.N, p.HW, p.C,
                                 gmode, st), 'pg_loss_grad')
    return buf


def loss_value_and_grad(p, y, tconst, mode, alpha, grad_out, loss_out, loss_slot, bglobal, beta=0.75, gamma=0.75,
                        allreduce=None):
    """Evaluate one loss term over prediction View p against target View y (or the constant tconst), write its
    value into loss_out[loss_slot] and, if grad_out is not None, its gradient wrt p into View grad_out.
    `allreduce(tensor)` starts the SUM of the two global reduction terms across ranks and returns wait()."""
    h = loss_begin(p, y, tconst, beta, allreduce, need_sums=mode in (L.LOSS_TVERSKY, L.LOSS_WBCE))
    return loss_finish(h, mode, alpha, grad_out, loss_out, loss_slot, bglobal, gamma)


REFERENCE_LOSSES = ('tversky', 'weighted_bce', 'MAE')      # the reference's objectives: pg_loss_reduce_parts / pg_loss_value_grad
SEG_OBJECTIVES = ('ce', 'focal', 'dice')                   # Trainer.loss_type beyond them, alone or '+'-joined: segloss.hip
_SEG_BITS = {'ce': L.SEG_CE, 'focal': L.SEG_FOCAL, 'dice': L.SEG_DICE}


class SegLossSpec(tuple):
    """check_seg_loss's result for a new objective: (terms, focal_gamma, focal_alpha, dice_smooth) -- the PG_SEG_* mask and the settings
    as the entry points take them (focal_alpha None -> PG_SEG_FOCAL_ALPHA_NONE) -- and, with per-class weights set, a fifth member: the
    weights as a tuple of fp32-rounded floats (without weights the tuple is the four-member one).  Hashable: it is part of the step's
    kind key.  `cw` is the weights' device buffer (None without weights, or where check_seg_loss was given no device): an attribute,
    not part of the value."""
    cw = None
    terms = property(lambda s: s[0])
    focal_gamma = property(lambda s: s[1])
    focal_alpha = property(lambda s: s[2])
    dice_smooth = property(lambda s: s[3])
    class_weights = property(lambda s: s[4] if len(s) > 4 else None)


CLASS_WEIGHT_SCHEMES = ('balanced', 'balanced_sqrt')


def check_class_weights(class_weights, C):
    """Per-class weights validated: None, or a sequence of C numbers, each finite and >= 0 as an fp32 number, at least one > 0 ->
    None or the tuple of fp32-rounded floats.  ValueError otherwise -- also for a scheme name ('balanced' | 'balanced_sqrt'), which
    stands for weights that have not been estimated yet (Trainer.estimate_class_weights)."""
    if class_weights is None:
        return None
    if isinstance(class_weights, str):
        if class_weights in CLASS_WEIGHT_SCHEMES:
            raise ValueError(f"class_weights = {class_weights!r} has not been resolved yet: call estimate_class_weights(data) (train() "
                             f"does before its first epoch)")
        raise ValueError(f"class_weights must be None, a sequence of {C} numbers or one of {' | '.join(CLASS_WEIGHT_SCHEMES)}, "
                         f"not {class_weights!r}")
    try:
        ws = list(class_weights)
    except TypeError:
        raise ValueError(f"class_weights must be None or a sequence of {C} numbers, not {class_weights!r}") from None
    if len(ws) != int(C):
        raise ValueError(f"class_weights has {len(ws)} entries for {C} output channels")
    out = []
    for w in ws:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError(f"class_weights must be numbers, not {w!r}")
        f = _f32(w)
        if not math.isfinite(f) or not f >= 0.0:
            raise ValueError(f"class_weights: {w!r} is not a finite fp32 number >= 0")
        out.append(f)
    if not any(f > 0.0 for f in out):
        raise ValueError("class_weights: at least one weight must be > 0 as an fp32 number")
    return tuple(out)


def class_weights_from_counts(counts, scheme='balanced'):
    """Weights from per-class pixel counts n_c (the first C words of pg_seg_label_count's result), in float64, rounded to fp32 at the
    end: f_c = n_c / sum_k n_k; r_c = 1 / f_c ('balanced') or 1 / sqrt(f_c) ('balanced_sqrt'); a class that does not occur takes the
    largest r among those that do; w = r * C / sum r (the mean weight is 1).  -> a list of C floats.  ValueError for C == 1, for counts
    that are all zero, a negative count or an unknown scheme."""
    if scheme not in CLASS_WEIGHT_SCHEMES:
        raise ValueError(f"scheme must be one of {' | '.join(CLASS_WEIGHT_SCHEMES)}, not {scheme!r}")
    n = np.asarray(counts, dtype=np.float64).reshape(-1)
    C = n.size
    if C < 2:
        raise ValueError("class weights need at least two classes (one channel has nothing to be balanced against)")
    if not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError(f"counts must be finite and >= 0, not {list(counts)!r}")
    total = n.sum()
    if not total > 0:
        raise ValueError("class weights from counts that are all zero")
    seen = n > 0
    f = n[seen] / total
    r = np.empty(C, dtype=np.float64)
    r[seen] = 1.0 / f if scheme == 'balanced' else 1.0 / np.sqrt(f)
    r[~seen] = r[seen].max()
    w = r * C / r.sum()
    return [float(x) for x in w.astype(np.float32)]


_SEG_WEIGHT_BUFFERS = {}      # (weights, device) -> the weights' device buffer, most recently used last
_SEG_WEIGHT_BUFFERS_MAX = 16


def seg_weight_buffer(weights, device):
    """The device buffer (C floats) of a weights tuple, made on first use -- the one host-to-device copy; a step that has checked its
    settings up front (Trainer.batch does, ahead of any capture) finds it here.  A captured step keeps its buffer alive itself."""
    key = (weights, str(torch.device(device)))
    t = _SEG_WEIGHT_BUFFERS.pop(key, None)
    if t is None:
        t = torch.tensor(weights, dtype=torch.float32).to(device)
    _SEG_WEIGHT_BUFFERS[key] = t
    while len(_SEG_WEIGHT_BUFFERS) > _SEG_WEIGHT_BUFFERS_MAX:
        _SEG_WEIGHT_BUFFERS.pop(next(iter(_SEG_WEIGHT_BUFFERS)))
    return t


def check_seg_loss(loss_type, final_act, C, focal_gamma=2, focal_alpha=None, dice_smooth=1.0, class_weights=None, device=None):
    """Trainer.loss_type and its settings against the generator's head (final_act) and channel count C, validated.  None for one of the
    reference's three names ("not ours": the existing kernels, whatever the settings hold); a SegLossSpec for 'ce', 'focal', 'dice' or
    a '+'-joined sum of them.  ValueError for an unknown name, a repeated or mixed sum, a head that does not give probabilities in
    [0, 1] (ce: softmax only, on at least two channels) and a bad setting.
    class_weights: None, or C numbers, finite and >= 0 as fp32 numbers with at least one > 0 (check_class_weights); with one of the
    reference's three names anything but None is a ValueError (they have no per-class weights: the setting would be silently inert).
    With `device` the spec carries the weights' device buffer (spec.cw)."""
    names = ' | '.join(REFERENCE_LOSSES + SEG_OBJECTIVES)
    if not isinstance(loss_type, str):
        raise ValueError(f"loss_type must be one of {names} (the last three also '+'-joined, e.g. 'ce+dice'), not {loss_type!r}")
    if loss_type in REFERENCE_LOSSES:
        if class_weights is not None:
            raise ValueError(f"class_weights needs loss_type = {' | '.join(SEG_OBJECTIVES)} or a sum of them; loss_type = {loss_type!r} "
                             f"has no per-class weights")
        return None
    members = loss_type.split('+')
    for m in members:
        if m in REFERENCE_LOSSES:
            raise ValueError(f"loss_type = {loss_type!r}: {m!r} does not combine with other objectives (sums are made of "
                             f"{' | '.join(SEG_OBJECTIVES)} only)")
        if m not in SEG_OBJECTIVES:
            raise ValueError(f"loss_type must be one of {names} (the last three also '+'-joined, e.g. 'ce+dice'), not {loss_type!r}")
    if len(set(members)) != len(members):
        raise ValueError(f"loss_type = {loss_type!r}: each objective may be used once in a sum")
    if isinstance(focal_gamma, bool) or not isinstance(focal_gamma, int) or not 0 <= focal_gamma <= L.SEG_FOCAL_GAMMA_MAX:
        raise ValueError(f"focal_gamma must be an integer in 0 .. {L.SEG_FOCAL_GAMMA_MAX} (the powers are repeated multiplications), "
                         f"not {focal_gamma!r}")
    if focal_alpha is not None and (isinstance(focal_alpha, bool) or not isinstance(focal_alpha, (int, float))
                                    or not 0.0 < float(focal_alpha) < 1.0):
        raise ValueError(f"focal_alpha must be None or a number in (0, 1), not {focal_alpha!r}")
    if (isinstance(dice_smooth, bool) or not isinstance(dice_smooth, (int, float)) or not math.isfinite(float(dice_smooth))
            or not float(dice_smooth) > 0.0):
        raise ValueError(f"dice_smooth must be a finite number > 0, not {dice_smooth!r}")
    if focal_alpha is not None and not 0.0 < _f32(focal_alpha) < 1.0:
        raise ValueError(f"focal_alpha = {focal_alpha!r} is not inside (0, 1) as an fp32 number")
    if not (0.0 < _f32(dice_smooth) < math.inf):
        raise ValueError(f"dice_smooth = {dice_smooth!r} is not a finite fp32 number > 0")
    if 'ce' in members and final_act != 'softmax':
        raise ValueError(f"loss_type = {loss_type!r}: 'ce' is categorical cross-entropy and needs a generator with final_act='softmax', "
                         f"not {final_act!r}")
    if 'ce' in members and int(C) < 2:
        raise ValueError(f"loss_type = {loss_type!r}: 'ce' needs at least two output channels, not {C}")
    if final_act not in ('softmax', 'sigmoid'):
        raise ValueError(f"loss_type = {loss_type!r} needs probabilities in [0, 1]: a generator with final_act='sigmoid' or 'softmax', "
                         f"not {final_act!r}")
    terms = 0
    for m in members:
        terms |= _SEG_BITS[m]
    base = (terms, int(focal_gamma), float(focal_alpha) if focal_alpha is not None else None, float(dice_smooth))
    weights = check_class_weights(class_weights, C)
    if weights is None:
        return SegLossSpec(base)
    spec = SegLossSpec(base + (weights,))
    if device is not None:
        spec.cw = seg_weight_buffer(weights, device)
    return spec


def _f32(x):
    """x as the fp32 number a launch argument carries."""
    with np.errstate(over='ignore'):
        return float(np.float32(x))


class SegLossBuffers:
    """Scratch for one evaluation of the new objectives: ws, the partial slabs pg_seg_loss_reduce writes and pg_seg_loss_value_grad
    adds.  Kept alive by the caller until both launches are enqueued; nothing reads it afterwards."""

    def __init__(self, N, HW, C, device):
        self.nbytes = int(L.load().pg_seg_loss_workspace_bytes(N, HW, C))
        self.ws = torch.empty(self.nbytes // 8, dtype=torch.float64, device=device)


class PendingSegLoss:
    """An evaluation of the new objectives between its two launches."""
    __slots__ = ('buf', 'args')


def seg_loss_begin(p, y, spec):
    """Phase 1 of Trainer.loss_type = 'ce' | 'focal' | 'dice' | a sum, over prediction View p against target View y: ONE launch
    (pg_seg_loss_reduce), the counterpart of loss_begin.  spec: check_seg_loss's result.  Nothing is exchanged under data parallelism:
    the objectives are means over samples."""
    assert not p.bf and not y.bf and (y.N, y.HW, y.C) == (p.N, p.HW, p.C)
    h = PendingSegLoss()
    h.buf, h.args = SegLossBuffers(p.N, p.HW, p.C, p.t.device), (p, y, spec)
    alpha = spec.focal_alpha if spec.focal_alpha is not None else L.SEG_FOCAL_ALPHA_NONE
    L.check(L.load().pg_seg_loss_reduce(p.ptr(), p.ld, y.ptr(), y.ld, p.N, p.HW, p.C, spec.terms, spec.focal_gamma, alpha,
                                        h.buf.ws.data_ptr(), h.buf.nbytes, _stream()), 'pg_seg_loss_reduce')
    return h


def seg_loss_finish(h, alpha, grad_out, loss_out, loss_slot, bglobal):
    """Phase 2: ONE launch (pg_seg_loss_value_grad) writes the value -- this rank's partial of the global mean, seg_alpha times the sum
    of the members -- into loss_out[loss_slot] and, if grad_out is not None, the gradient wrt p into View grad_out, seeded for the SUM
    all-reduce.  Returns the scratch buffers (not a result), as loss_finish does."""
    p, y, spec = h.args
    assert grad_out is None or (not grad_out.bf and (grad_out.N, grad_out.HW, grad_out.C) == (p.N, p.HW, p.C))
    a, b, hw, c = float(alpha), float(bglobal), float(p.HW), float(p.C)
    fa = spec.focal_alpha if spec.focal_alpha is not None else L.SEG_FOCAL_ALPHA_NONE
    gp, gl = _pl(grad_out)
    if spec.class_weights is not None:
        # per-class weights: the same launch with the weights' device buffer (made with the spec: no copy in here)
        cw = spec.cw if spec.cw is not None else seg_weight_buffer(spec.class_weights, p.t.device)
        assert cw.device == p.t.device and cw.numel() == p.C
        L.check(L.load().pg_seg_loss_value_grad_w(h.buf.ws.data_ptr(), h.buf.nbytes, p.ptr(), p.ld, y.ptr(), y.ld, p.N, p.HW, p.C,
                                                  spec.terms, spec.focal_gamma, fa, spec.dice_smooth, a / (b * hw), a / (b * c * hw),
                                                  a / (b * c), cw.data_ptr(), gp, gl, L.ptr(loss_out, loss_slot), _stream()),
                'pg_seg_loss_value_grad_w')
        h.buf.cw = cw      # (alive until the launch has run, with the scratch)
        return h.buf
    L.check(L.load().pg_seg_loss_value_grad(h.buf.ws.data_ptr(), h.buf.nbytes, p.ptr(), p.ld, y.ptr(), y.ld, p.N, p.HW, p.C, spec.terms,
                                            spec.focal_gamma, fa, spec.dice_smooth, a / (b * hw), a / (b * c * hw), a / (b * c),
                                            gp, gl, L.ptr(loss_out, loss_slot), _stream()), 'pg_seg_loss_value_grad')
    return h.buf


def seg_label_count(y, counts):
    """Add the per-class pixel counts of target View y to `counts` (int64 [C + 2] on the device: C classes, unlabelled, pixels): ONE
    launch (pg_seg_label_count), nothing read back."""
    assert not y.bf and counts.dtype == torch.int64 and counts.numel() == y.C + 2 and counts.is_contiguous()
    L.check(L.load().pg_seg_label_count(y.ptr(), y.ld, y.N, y.HW, y.C, counts.data_ptr(), _stream()), 'pg_seg_label_count')


GAN_MODES = ('vanilla', 'lsgan', 'hinge')


def check_gan_mode(gan_mode, real_label, final_act):
    """Trainer.gan_mode / real_label against the discriminator's head, validated: -> (gan_mode, float(real_label)).  ValueError for an
    unknown mode, a real label outside (0, 1], hinge on a sigmoid head (margins at +-1 mean nothing on (0, 1)) or with a smoothed label."""
    if not isinstance(gan_mode, str) or gan_mode not in GAN_MODES:
        raise ValueError(f"gan_mode must be one of {' | '.join(GAN_MODES)}, not {gan_mode!r}")
    if isinstance(real_label, bool) or not isinstance(real_label, (int, float)) or not 0.0 < float(real_label) <= 1.0:
        raise ValueError(f"real_label must be a number in (0, 1], not {real_label!r}")
    if gan_mode == 'hinge' and final_act != 'none':
        raise ValueError("gan_mode = 'hinge' needs a discriminator that returns logits (Discriminator(final_act='none')): "
                         "margins at +-1 mean nothing on a sigmoid's (0, 1)")
    if gan_mode == 'hinge' and float(real_label) != 1.0:
        raise ValueError(f"gan_mode = 'hinge' takes no label smoothing: real_label must be 1, not {real_label!r}")
    return gan_mode, float(real_label)


def gan_kinds(gan_mode, final_act):
    """(generator term, discriminator terms): the PG_GAN_* kind of pg_gan_loss for each, None where the step keeps PG_LOSS_BCE
    (vanilla on a sigmoid head)."""
    if gan_mode == 'hinge':
        return L.GAN_HINGE_G, L.GAN_HINGE_D
    if gan_mode == 'lsgan':
        return L.GAN_LSGAN, L.GAN_LSGAN
    return (L.GAN_BCE_LOGITS, L.GAN_BCE_LOGITS) if final_act == 'none' else (None, None)


def gan_loss(terms, loss_out, bglobal):
    """Up to GAN_MAX_TERMS terms in ONE pg_gan_loss call.  terms: (d, kind, target, alpha, grad, slot) -- d a one-channel patch View,
    grad a View of its shape or None (value only), the value alpha * sum e / (bglobal * HW) going to loss_out[slot] (this rank's partial
    of the global mean) and the gradient seeded with the same factor.  Returns the workspace of the partial-slab path (None on the
    one-launch path): scratch the caller keeps until the launches are enqueued."""
    lib = L.load()
    items = (L.GanTerm * len(terms))()
    for it, (d, kind, target, alpha, grad, slot) in zip(items, terms):
        assert d.C == 1 and not d.bf and (grad is None or (grad.C == 1 and grad.npix == d.npix and not grad.bf))
        it.d, it.ld, it.n, it.kind, it.target = d.ptr(), d.ld, d.npix, kind, float(target)
        it.scale = float(alpha) / (float(bglobal) * float(d.HW))
        it.g, it.ld_g = (grad.ptr(), grad.ld) if grad is not None else (None, 0)
        it.value = L.ptr(loss_out, slot)
    nb = int(lib.pg_gan_loss_workspace_bytes(len(terms), items))
    ws = torch.empty(nb // 8, dtype=torch.float64, device=loss_out.device) if nb else None
    L.check(lib.pg_gan_loss(len(terms), items, ws.data_ptr() if ws is not None else None, nb, _stream()), 'pg_gan_loss')
    return ws
