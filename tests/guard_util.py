"""Guarded device buffers for the containment tests: every kernel may write only what the caller handed it.

One torch.uint8 tensor filled with byte 0xFF holds a front guard (>= 4 KiB), an inner region that starts at a 256-byte-aligned
address, and a back guard.  All-ones is a NaN as fp32, bf16 and fp64: it poisons a read of memory the kernel was not given, and no
kernel produces it as a computed NaN (the hardware's NaNs are 0x7FC0.. / 0xFFC0.., never all ones) -- so a byte that is no longer 0xFF was
written.  The checks are exact byte comparisons, one device-side reduction each; the decode of an offending offset runs only on
failure."""
import torch

from patchgan_amd import engine as E

DEV = 'cuda'
SENTINEL = 0xFF
FRONT = 4096          # bytes of guard before the inner region (rounded up to the next 256-byte-aligned address)
BACK = 4096           # default bytes of guard after it


class Guarded:
    """`nbytes` of device memory between two guards.  kind 'flat': the first `written` bytes may change; kind 'view': an NHWC
    tensor of pixel stride ld (elements of `es` bytes) of which only channels [off, off + C) of each pixel may change."""

    def __init__(self, nbytes, back=BACK, device=None):
        nbytes, back = int(nbytes), max(int(back), BACK)
        self.raw = torch.full((FRONT + 256 + nbytes + back,), SENTINEL, dtype=torch.uint8, device=device or DEV)
        self.lo = FRONT + (-(self.raw.data_ptr() + FRONT)) % 256
        self.nbytes = nbytes
        self.kind = 'flat'
        self.ld = self.off = self.C = self.es = self.shape = None
        assert (self.raw.data_ptr() + self.lo) % 256 == 0 and self.lo + nbytes + back <= self.raw.numel()

    def ptr(self):
        return self.raw.data_ptr() + self.lo

    def inner(self, dtype=torch.uint8):
        """The inner region as a tensor of `dtype` (shares memory with the guarded buffer)."""
        return self.raw[self.lo:self.lo + self.nbytes].view(dtype)

    def snapshot(self):
        return self.raw.clone()


def flat(nbytes, back=BACK):
    """Guarded flat buffer of exactly nbytes, all sentinel (an output: dP, dbias, part, u_cache, v_keep, a workspace, ...)."""
    return Guarded(nbytes, back)


def flat_from(t, back=BACK):
    """Guarded flat buffer holding exactly the bytes of tensor `t` (an input: weights, bias, coefficients, ...)."""
    t = t.contiguous().to(DEV)
    g = Guarded(t.numel() * t.element_size(), back)
    g.inner(t.dtype).copy_(t.reshape(-1))
    return g


def view(N, H, W, C, ld=None, off=0, bf=False, back=BACK):
    """(engine.View, Guarded): an NHWC channel slice (fp32 or bf16, pixel stride ld, channel offset off) inside a guarded buffer of
    exactly N*H*W*ld elements, the whole of it sentinel."""
    ld = ld or C
    assert 0 <= off and off + C <= ld
    es = 2 if bf else 4
    g = Guarded(N * H * W * ld * es, back)
    g.kind, g.ld, g.off, g.C, g.es, g.shape = 'view', ld, off, C, es, (N, H, W)
    v = E.View(g.inner(torch.bfloat16 if bf else torch.float32), off, ld, N, H, W, C, bf)
    assert v.ptr() == g.ptr() + off * es
    return v, g


def load_nchw(v, x, pad=None):
    """Fill ONLY the slice of view v from an NCHW tensor (torch indexing: no kernel of the library under test).  pad: a value for
    every other channel of the pixels (8-channel bf16 pixels carry zeros there by contract)."""
    t = v.t[:v.npix * v.ld].view(v.N, v.H, v.W, v.ld)
    if pad is not None:
        t.fill_(pad)
    t[..., v.off:v.off + v.C] = x.to(t.device).permute(0, 2, 3, 1).to(t.dtype)
    return v


def view_from(x, ld=None, off=0, bf=False, pad=None):
    """Guarded view holding the NCHW tensor x in its slice (an input)."""
    N, C, H, W = x.shape
    v, g = view(N, H, W, C, ld, off, bf)
    load_nchw(v, x, pad)
    return v, g


def read_nchw(v):
    """The slice of view v as a float64 NCHW tensor (torch indexing)."""
    return v.t[:v.npix * v.ld].view(v.N, v.H, v.W, v.ld)[..., v.off:v.off + v.C].permute(0, 3, 1, 2).double()


def _allowed(g, written):
    """Byte mask over g.raw of what the call may have written."""
    ok = torch.zeros(g.raw.numel(), dtype=torch.bool, device=g.raw.device)
    if written is None:
        return ok
    if g.kind == 'flat':
        nb = g.nbytes if written == 'all' else int(written)
        assert 0 <= nb <= g.nbytes
        ok[g.lo:g.lo + nb] = True
        return ok
    c0, c1 = (g.off, g.off + g.C) if written == 'slice' else (0, g.ld) if written == 'all' else written
    assert 0 <= c0 <= c1 <= g.ld
    ok[g.lo:g.lo + g.nbytes].view(-1, g.ld * g.es)[:, c0 * g.es:c1 * g.es] = True
    return ok


def where(g, index, written=None):
    """Byte index into g.raw -> words: front guard / back guard / beyond nbytes / (pixel, channel)."""
    o = int(index) - g.lo
    if o < 0:
        return f'front guard, {-o} bytes before the region'
    if o >= g.nbytes:
        return f'back guard, byte {o - g.nbytes} after the region of {g.nbytes} bytes'
    if g.kind == 'flat':
        return f'byte {o} of the region, beyond nbytes = {written if written is not None else 0} (region {g.nbytes} bytes)'
    pix, rem = divmod(o, g.ld * g.es)
    N, H, W = g.shape
    n, hw = divmod(pix, H * W)
    return (f'pixel {pix} (n={n}, h={hw // W}, w={hw % W}), channel {rem // g.es} of ld {g.ld} '
            f'(slice is channels {g.off}..{g.off + g.C - 1}), byte {rem % g.es} of the element')


def assert_untouched(g, written=None, what=''):
    """Every byte of g outside the declared written set is still the sentinel.  written: None (nothing); flat buffers: a byte count
    (the first `written` bytes of the region) or 'all'; views: 'slice' (the slice's channels of each pixel), 'all', or a channel
    range (c0, c1) of each pixel."""
    bad = (g.raw != SENTINEL) & ~_allowed(g, written)
    if bool(bad.any().item()):              # the one reduction of the passing case
        first = int(bad.nonzero()[0].item())
        raise AssertionError(f'{what}: {int(bad.sum().item())} bytes written outside the declared set, first at {where(g, first, written)}')


def assert_unchanged(g, snap, what=''):
    """An input buffer is byte-identical to its snapshot (guards included)."""
    if not torch.equal(g.raw, snap):
        first = int((g.raw != snap).nonzero()[0].item())
        raise AssertionError(f'{what}: input buffer modified, first at {where(g, first)}')


class Inputs:
    """The input buffers of one call with their snapshots: check() asserts that none of them changed."""

    def __init__(self):
        self.items = []

    def add(self, g, name):
        if g is not None:
            self.items.append((g, g.snapshot(), name))
        return g

    def check(self, what=''):
        for g, snap, name in self.items:
            assert_unchanged(g, snap, f'{what} input {name}')
