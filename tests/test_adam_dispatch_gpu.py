"""engine.adam_update on the device: for all 16 combinations of (device scalars, weight average, status block, weight decay) one
update leaves p, m, v (and the average) bit for bit what the entry point of tests/test_adam_dispatch_cpu.py's table leaves when it is
called directly through ctypes on copies of the same state.  Sizes: 1 (tail only), 7 (one float4 and a 3-element tail), 1029 (many
threads of vector body and a 1-element tail); step 3 and betas (0.5, 0.99), so a swapped beta or a wrong bias correction shows; a
host-built status block with apply = 1, coef = 0.5, and one with apply = 0, which must leave every buffer's bits alone.
Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

from tests.test_adam_dispatch_cpu import COMBOS, TABLE, _ids

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NS = (1, 7, 1029)
STEP, LR, B1, B2, EPS, EMA_DECAY, WD = 3, 2e-3, 0.5, 0.99, 1e-8, 0.75, 0.125


def _state(n):
    """(p, g, m, v, ema) on the host, fixed by n: a state a few steps into training (m != 0, v > 0)."""
    gen = torch.Generator().manual_seed(1000 + n)
    p, g, m, ema = (torch.randn(n, generator=gen) for _ in range(4))
    return p, g, 0.1 * m, torch.rand(n, generator=gen) + 0.01, ema


def _stat(apply, coef=0.5):
    from patchgan_amd import engine as E
    rec = np.zeros(1, dtype=E.GRAD_STAT)
    rec['coef'], rec['apply'], rec['norm'] = coef, apply, 2.0
    return torch.from_numpy(rec.view(np.float64).copy()).to(DEV)


def _scalars(wd):
    from patchgan_amd import engine as E
    return torch.tensor([float(x) for x in E.adam_scalars(STEP, LR, B1, B2, WD if wd else None)], dtype=torch.float32, device=DEV)


def _direct(lib, name, bufs, scal, stat):
    """The entry point `name` called as the C header declares it, every argument spelt here."""
    p, g, m, v, ema = bufs
    ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    n, eptr, sptr = p.numel(), (ema.data_ptr() if ema is not None else None), (stat.data_ptr() if stat is not None else None)
    decay = EMA_DECAY if ema is not None else 0.0
    bc1, sbc2, dm = 1.0 - B1 ** STEP, math.sqrt(1.0 - B2 ** STEP), 1.0 - LR * WD
    sc = scal.data_ptr() if scal is not None else None
    calls = {
        'pg_adam_step': lambda: lib.pg_adam_step(*ptrs, n, LR, B1, B2, EPS, bc1, sbc2, None),
        'pg_adam_step_dev': lambda: lib.pg_adam_step_dev(*ptrs, n, B1, B2, EPS, sc, None),
        'pg_adam_ema_step': lambda: lib.pg_adam_ema_step(*ptrs, eptr, n, LR, B1, B2, EPS, bc1, sbc2, decay, None),
        'pg_adam_ema_step_dev': lambda: lib.pg_adam_ema_step_dev(*ptrs, eptr, n, B1, B2, EPS, sc, decay, None),
        'pg_adam_clip_step': lambda: lib.pg_adam_clip_step(*ptrs, eptr, n, LR, B1, B2, EPS, bc1, sbc2, decay, sptr, None),
        'pg_adam_clip_step_dev': lambda: lib.pg_adam_clip_step_dev(*ptrs, eptr, n, B1, B2, EPS, sc, decay, sptr, None),
        'pg_adamw_step': lambda: lib.pg_adamw_step(*ptrs, eptr, n, LR, B1, B2, EPS, bc1, sbc2, dm, decay, sptr, None),
        'pg_adamw_step_dev': lambda: lib.pg_adamw_step_dev(*ptrs, eptr, n, B1, B2, EPS, sc, decay, sptr, None),
    }
    assert calls[name]() == 0, name


def _both(combo, n, apply):
    """-> (the host state, buffers after engine.adam_update, buffers after the table's entry point), absent buffers None."""
    from patchgan_amd import _lib as L, engine as E
    dev, ema, stat, wd = combo
    host = _state(n)
    out = []
    for via_engine in (True, False):
        bufs = [x.to(DEV) for x in host[:4]] + [host[4].to(DEV) if ema else None]
        assert all(x is None or x.data_ptr() % 16 == 0 for x in bufs)
        st = _stat(apply) if stat else None
        scal = _scalars(wd) if dev else None
        if via_engine:
            when = dict(scalars=scal) if dev else dict(step=STEP, lr=LR)
            E.adam_update(*bufs[:4], ema=bufs[4], ema_decay=EMA_DECAY if ema else None, stat=st, weight_decay=WD if wd else None,
                          beta1=B1, beta2=B2, eps=EPS, **when)
        else:
            _direct(L.load(), TABLE[combo], bufs, scal, st)
        torch.cuda.synchronize()
        out.append([x.cpu() if x is not None else None for x in bufs])
    return (host,) + tuple(out)


def _bits(a, b):
    return torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('combo', COMBOS, ids=_ids)
def test_adam_update_is_the_tables_entry_point(combo):
    for n in NS:
        host, got, want = _both(combo, n, apply=1)
        for name, h, a, b in zip(('p', 'g', 'm', 'v', 'ema'), host, got, want):
            if a is None:
                assert b is None and name == 'ema' and not combo[1]
                continue
            assert _bits(a, b), (n, name)
            # (the update ran: every output moved, the gradient is only read)
            assert _bits(a, h) == (name == 'g'), (n, name)


@pytest.mark.parametrize('dev', [False, True], ids=['args', 'dev_scalars'])
def test_a_block_that_says_skip_keeps_every_bit(dev):
    for n in NS:
        host, got, want = _both((dev, True, True, True), n, apply=0)
        for name, h, a, b in zip(('p', 'g', 'm', 'v', 'ema'), host, got, want):
            assert _bits(a, h) and _bits(b, h), (n, name)
