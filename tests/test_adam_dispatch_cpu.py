"""engine.adam_update, the one Python wrapper of the eight pg_adam* entry points, without a GPU: for all 16 combinations of (device
scalars, weight average, status block, weight decay) a recording stand-in for the library shows which entry point is called and with
exactly which arguments.  The expected names are written out below, not computed by engine.adam_entry."""
import ctypes
import math

import pytest
import torch

# (dev, ema, stat, weight_decay) -> entry point: a decay wins over a status block, which wins over an average
TABLE = {
    (False, False, False, False): 'pg_adam_step',
    (False, True, False, False): 'pg_adam_ema_step',
    (False, False, True, False): 'pg_adam_clip_step',
    (False, True, True, False): 'pg_adam_clip_step',
    (False, False, False, True): 'pg_adamw_step',
    (False, True, False, True): 'pg_adamw_step',
    (False, False, True, True): 'pg_adamw_step',
    (False, True, True, True): 'pg_adamw_step',
    (True, False, False, False): 'pg_adam_step_dev',
    (True, True, False, False): 'pg_adam_ema_step_dev',
    (True, False, True, False): 'pg_adam_clip_step_dev',
    (True, True, True, False): 'pg_adam_clip_step_dev',
    (True, False, False, True): 'pg_adamw_step_dev',
    (True, True, False, True): 'pg_adamw_step_dev',
    (True, False, True, True): 'pg_adamw_step_dev',
    (True, True, True, True): 'pg_adamw_step_dev',
}
COMBOS = sorted(TABLE)
STEP, LR, B1, B2, EPS, EMA_DECAY, WD = 3, 2e-3, 0.5, 0.99, 1e-7, 0.75, 0.125


class _Lib:
    """Stands in for the loaded library: every pg_* attribute records its call and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('pg_'):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.fixture
def lib(monkeypatch):
    from patchgan_amd import _lib as L, engine as E
    stand_in = _Lib()
    monkeypatch.setattr(L, 'load', lambda: stand_in)
    monkeypatch.setattr(E, '_stream', lambda: 'STREAM')
    return stand_in


def _buffers(n=7):
    return {k: torch.zeros(n) for k in ('p', 'g', 'm', 'v', 'ema', 'scalars')}, torch.zeros(8, dtype=torch.float64)


def _ids(c):
    return '-'.join(name for name, on in zip(('dev', 'ema', 'stat', 'wd'), c) if on) or 'plain'


def test_the_table_is_the_rule_adam_entry_states():
    from patchgan_amd import engine as E
    assert len(TABLE) == 16
    for (dev, ema, stat, wd), name in TABLE.items():
        assert E.adam_entry(ema, stat, wd, dev) == name
        assert E.adam_entry(ema=ema, stat=stat, weight_decay=wd, dev=dev) == name


@pytest.mark.parametrize('combo', COMBOS, ids=_ids)
def test_entry_point_and_arguments(lib, combo):
    from patchgan_amd import _lib as L, engine as E
    dev, ema, stat, wd = combo
    b, st = _buffers()
    kw = dict(scalars=b['scalars']) if dev else dict(step=STEP, lr=LR)
    E.adam_update(b['p'], b['g'], b['m'], b['v'], ema=b['ema'] if ema else None, ema_decay=EMA_DECAY if ema else None,
                  stat=st if stat else None, weight_decay=WD if wd else None, beta1=B1, beta2=B2, eps=EPS, **kw)
    (name, args), = lib.calls
    assert name == TABLE[combo]
    family = name[len('pg_'):].replace('_dev', '')
    ema_ptr = b['ema'].data_ptr() if ema else None
    want = [b['p'].data_ptr(), b['g'].data_ptr(), b['m'].data_ptr(), b['v'].data_ptr()]
    if family != 'adam_step':
        want.append(ema_ptr)
    want.append(7)
    if dev:
        want += [B1, B2, EPS, b['scalars'].data_ptr()]
    else:
        want += [LR, B1, B2, EPS, 1.0 - B1 ** STEP, math.sqrt(1.0 - B2 ** STEP)]
        if family == 'adamw_step':
            want.append(E.decay_mul(LR, WD))
    if family != 'adam_step':
        want.append(EMA_DECAY if ema else 0.0)
    if family in ('adam_clip_step', 'adamw_step'):
        want.append(st.data_ptr() if stat else None)
    want.append('STREAM')
    assert list(args) == want and [type(x) for x in args] == [type(x) for x in want]
    # ... which is one value per parameter of the C signature, of a kind ctypes converts to it
    argtypes = L.SIGNATURES[name][1]
    assert len(args) == len(argtypes)
    for x, ct in zip(args[:-1], argtypes[:-1]):
        if ct is ctypes.c_void_p:
            assert x is None or isinstance(x, int)
        elif ct is ctypes.c_long:
            assert isinstance(x, int)
        else:
            assert ct is ctypes.c_float and isinstance(x, float)
    assert argtypes[-1] is ctypes.c_void_p


def test_the_defaults_are_torch_adams(lib):
    from patchgan_amd import engine as E
    b, _ = _buffers()
    E.adam_update(b['p'], b['g'], b['m'], b['v'], step=1, lr=1e-3)
    (name, args), = lib.calls
    assert name == 'pg_adam_step' and args[5:11] == (1e-3, 0.9, 0.999, 1e-8, 1.0 - 0.9 ** 1, math.sqrt(1.0 - 0.999 ** 1))


def test_a_failing_launch_raises_with_the_entry_points_name(lib, monkeypatch):
    from patchgan_amd import _lib as L, engine as E
    b, _ = _buffers()
    monkeypatch.setattr(L, 'load', lambda: type('Refusing', (), {'pg_adamw_step_dev': staticmethod(lambda *a: 1)})())
    with pytest.raises(RuntimeError, match='pg_adamw_step_dev failed'):
        E.adam_update(b['p'], b['g'], b['m'], b['v'], scalars=b['scalars'], weight_decay=WD)


@pytest.mark.parametrize('kw', [dict(), dict(step=3), dict(lr=1e-3), dict(step=3, lr=1e-3, scalars=True), dict(step=3, scalars=True),
                                dict(lr=1e-3, scalars=True)],
                         ids=['neither', 'step_alone', 'lr_alone', 'both', 'step_and_scalars', 'lr_and_scalars'])
def test_step_and_lr_or_scalars(lib, kw):
    from patchgan_amd import engine as E
    b, _ = _buffers()
    if 'scalars' in kw:
        kw = dict(kw, scalars=b['scalars'])
    with pytest.raises(ValueError):
        E.adam_update(b['p'], b['g'], b['m'], b['v'], **kw)
    assert lib.calls == []


def test_a_decay_that_flips_the_weights_is_refused_before_the_launch(lib):
    from patchgan_amd import engine as E
    b, _ = _buffers()
    with pytest.raises(ValueError):
        E.adam_update(b['p'], b['g'], b['m'], b['v'], step=1, lr=0.5, weight_decay=2.0)
    assert lib.calls == []
