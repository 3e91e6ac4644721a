"""Gradient accumulation (Trainer.accumulate) without a GPU: the C ABI of pg_grad_accum (argument validation happens before any launch),
the float32 replay of tests/accum_util.py against float64, the window's phase sequence, the YAML and attribute validation, and the
trainer's dispatch: which engine calls _adam_step makes in each phase, what moves the window and what discards it."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

from tests import accum_util as A
from tests import adam_spy as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
BAD_SETTINGS = (0, -1, 2.5, True, False, '2', (2,), NAN)


def _trainer(tmp_path, spectral=False, seed=3):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3, spectral_norm=spectral)
    return pg.Trainer(g, d, str(tmp_path))


# ---------------------------------------------------------------------------------------------- 1. C ABI
def test_symbol_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    for name, value in (('PG_ACC_BEGIN', A.BEGIN), ('PG_ACC_ADD', A.ADD), ('PG_ACC_CLOSE', A.CLOSE), ('PG_ACC_CLOSE_ONLY', A.CLOSE_ONLY)):
        assert re.search(rf'#define {name} {value}\b', src), name
    assert (_lib.ACC_BEGIN, _lib.ACC_ADD, _lib.ACC_CLOSE, _lib.ACC_CLOSE_ONLY) == (A.BEGIN, A.ADD, A.CLOSE, A.CLOSE_ONLY)
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    assert 'pg_grad_accum' in declared and hasattr(lib, 'pg_grad_accum') and 'pg_grad_accum' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['pg_grad_accum'][1]) == 6


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a, g = 1 << 20, 1 << 24           # non-NULL, 16-byte-aligned, 16 MiB apart, never dereferenced: every call below is refused on the host
    n = 4099

    def call(acc=a, g=g, n=n, mode=A.CLOSE, scale=0.5):
        return lib.pg_grad_accum(acc, g, n, mode, scale, None)
    for mode in (A.BEGIN, A.ADD, A.CLOSE, A.CLOSE_ONLY):
        assert call(acc=None, mode=mode) == -1 and call(g=None, mode=mode) == -1
        for off in (4, 8, 12):
            assert call(acc=a + off, mode=mode) == -1 and call(g=g + off, mode=mode) == -1, off
        for bad in (0, -1, -4099):
            assert call(n=bad, mode=mode) == -1
        # [acc, acc + n) and [g, g + n) intersect: the same buffer, g inside acc's range from either side, the last 16 bytes shared
        assert call(g=a, mode=mode) == -1
        assert call(g=a + 16, mode=mode) == -1 and call(acc=g + 16, mode=mode) == -1
        assert call(g=a + 4 * 4096, mode=mode) == -1 and call(acc=g + 4 * 4096, mode=mode) == -1
    for mode in (-1, 4, 17):
        assert call(mode=mode) == -1
    for mode in (A.CLOSE, A.CLOSE_ONLY):
        for bad in (NAN, INF, -INF, 0.0, -0.5, 1.0000001, 2.0):
            assert call(mode=mode, scale=bad) == -1, (mode, bad)


# ---------------------------------------------------------------------------------------------- 2. the replay
@pytest.mark.parametrize('k', (2, 4))
def test_replay_is_exact_on_dyadic_inputs(k):
    """Values j / 8 with |j| <= 2^12 and a scale of 1/2 or 1/4: every float32 sum and product of the replay is exact, so it must
    equal the float64 mean value for value -- in each mode and for the window as a whole."""
    for n in A.NS:
        grads = [A.dyadic(n, 10 * k + i) for i in range(k)]
        acc, closed = A.window(grads)
        assert closed.dtype == np.float32 and np.array_equal(closed.astype(np.float64), A.window_f64(grads))
        assert np.array_equal(acc.astype(np.float64), sum(g.astype(np.float64) for g in grads[:-1]))
        acc_s, closed_s = A.window(grads, short=True)
        assert np.array_equal(closed_s.astype(np.float64), A.window_f64(grads))
        assert np.array_equal(acc_s.astype(np.float64), sum(g.astype(np.float64) for g in grads))
    a, g = A.dyadic(9, 1), A.dyadic(9, 2)
    for mode in (A.BEGIN, A.ADD, A.CLOSE, A.CLOSE_ONLY):
        a1, g1 = A.replay(mode, a, g, 0.25)
        want_a = {A.BEGIN: g, A.ADD: a.astype(np.float64) + g}.get(mode, a)
        want_g = {A.CLOSE: (a.astype(np.float64) + g) * 0.25, A.CLOSE_ONLY: a.astype(np.float64) * 0.25}.get(mode, g)
        assert np.array_equal(a1.astype(np.float64), want_a) and np.array_equal(g1.astype(np.float64), want_g), mode


def test_replay_rounds_once_per_operation_and_propagates_specials():
    one, eps = np.float32(1.0), np.float32(2.0 ** -24)
    # (1 + 2^-24) rounds to 1 BEFORE the multiply: a fused (a + g) * s would keep the low bit
    _, closed = A.replay(A.CLOSE, [one], [eps], A.scale_of(3))
    assert closed[0] == one * A.scale_of(3)
    assert float(A.scale_of(3)) == float(np.float32(1.0 / 3.0)) and float(A.scale_of(2)) == 0.5
    g = np.float32(1.2345678)
    assert A.replay(A.CLOSE, [g], [g], A.scale_of(2))[1][0] == g          # (g + g) * 0.5f == g: the identity k = 2 has
    a = np.array([NAN, INF, -INF, 1.0, -0.0, 1e-40], dtype=np.float32)
    b = np.array([1.0, -INF, -INF, NAN, 0.0, 1e-40], dtype=np.float32)
    _, c = A.replay(A.CLOSE, a, b, 0.5)
    assert np.isnan(c[0]) and np.isnan(c[1]) and c[2] == -INF and np.isnan(c[3]) and c[4] == 0.0 and c[5] == np.float32(1e-40)
    assert A.same_bits(c, c.copy()) and not A.same_bits(np.float32([0.0]), np.float32([-0.0]))
    m = A.mixed(4099, 7)
    assert np.isnan(m).any() and np.isinf(m).any() and (np.abs(m[np.isfinite(m) & (m != 0)]) < 2.0 ** -126).any()


# ---------------------------------------------------------------------------------------------- 3. the phase sequence
def test_phase_sequence():
    from patchgan_amd import engine as E
    assert A.phases(2, 6) == ['begin', 'close'] * 3
    assert A.phases(3, 7) == ['begin', 'add', 'close'] * 2 + ['begin']
    assert A.phases(5, 10) == ['begin', 'add', 'add', 'add', 'close'] * 2
    # a discard in mid-window: the next call begins again
    assert A.phases(3, 6, discard_after=(2,)) == ['begin', 'add', 'begin', 'add', 'close', 'begin']
    assert A.phases(5, 7, discard_after=(1, 4)) == ['begin', 'begin', 'add', 'add', 'begin', 'add', 'add']
    for done, k in ((-1, 2), (2, 2), (5, 3)):
        with pytest.raises(ValueError):
            E.accum_phase(done, k)
    assert E.accum_scale(3).dtype == np.float32 and E.accum_scale(3) == A.scale_of(3)


# ---------------------------------------------------------------------------------------------- 4. settings
def test_yaml_and_attribute_validation(tmp_path):
    from patchgan_amd import engine as E, train as T
    assert T.accumulate_of(yaml.safe_load("accumulate: 4")['accumulate']) == 4
    assert T.accumulate_of(None) is None and T.accumulate_of(1) is None and T.accumulate_of(np.int64(3)) == 3
    assert T.accumulate_of(yaml.safe_load("accumulate: null")['accumulate']) is None
    for text in ("0", "-1", "2.5", "true", "'2'", "[2]", ".nan"):
        with pytest.raises(ValueError):
            T.accumulate_of(yaml.safe_load(f"accumulate: {text}")['accumulate'])
    for bad in BAD_SETTINGS:
        with pytest.raises(ValueError):
            E.check_accumulate(bad)
    t = _trainer(tmp_path)
    assert t.accumulate is None and t._acc_now() is None and t._acc_key() == ()
    T.apply_train_params(t, dict(loss_type='tversky', seg_alpha=200, accumulate=3))
    assert t.accumulate == 3 and t._acc_now() == 3
    T.apply_train_params(t, dict(loss_type='tversky', seg_alpha=200))
    assert t.accumulate is None
    with pytest.raises(ValueError):
        T.apply_train_params(t, dict(loss_type='tversky', seg_alpha=200, accumulate=0))
    # batch() refuses a bad setting at its top: before the inputs are looked at, before optimizers or buffers exist
    x = torch.zeros(1, 3, 256, 256)
    for bad in BAD_SETTINGS:
        t.accumulate = bad
        with pytest.raises(ValueError):
            t.batch(x, x[:, :1], train=True)
        with pytest.raises(ValueError):
            t.batch(x, x[:, :1], train=False)
        assert t._adam is None and t._acc is None
    for off in (None, 1):
        t.accumulate = off
        assert t._acc_now() is None and t._acc_begin_call() is None and not t._acc_ensure() and t._acc is None


def test_the_command_line_validates_before_it_builds_anything():
    """patchgan_train checks train_params.accumulate where it checks the other optimizer settings: ahead of the data sets and networks."""
    src = open(os.path.join(ROOT, 'patchgan_amd', 'train.py')).read()
    check = src.index("accumulate_of(config['train_params'].get('accumulate'))")
    assert src.index('parse_config(config)') < check < src.index("dataset_params.get('size'")
    assert check < src.index('Trainer(')


# ---------------------------------------------------------------------------------------------- 5. the trainer's dispatch
def _spied(monkeypatch):
    return S.spy(monkeypatch)


def _call(t):
    """What batch() does around one training step's two _adam_step calls, without the step."""
    acc = t._acc_cur = t._acc_begin_call()
    t._adam_step('g'), t._adam_step('d')
    t._acc_cur = None
    if acc is not None:
        t._acc_done = 0 if acc[0] == 'close' else acc[1]
    return acc


def test_dispatch_per_phase(tmp_path, monkeypatch):
    calls = _spied(monkeypatch)
    t = _trainer(tmp_path)
    t.setup_optimizers(1e-3, 2e-3)
    G, D = t.generator, t.discriminator
    G.ensure_grad_flat(), D.ensure_grad_flat()
    # off: the calls of before, nothing allocated
    for off in (None, 1):
        t.accumulate = off
        assert _call(t) is None
    assert [c[0] for c in calls] == ['adam_step'] * 4 and t._acc is None and (t._t_g, t._t_d) == (2, 2)
    del calls[:]
    t.setup_optimizers(1e-3, 2e-3)
    t.accumulate = 3
    assert _call(t) == ('begin', 1) and _call(t) == ('add', 2)
    assert [c[0] for c in calls] == ['grad_accum'] * 4 and (t._t_g, t._t_d) == (0, 0) and t._acc_done == 2
    assert [c[1][2] for c in calls] == ['begin', 'begin', 'add', 'add']
    assert calls[0][1][0] is t._acc[0] and calls[0][1][1] is G.grad_flat and calls[1][1][0] is t._acc[1] and calls[1][1][1] is D.grad_flat
    assert t._acc[0].shape == G.flat.shape and t._acc[1].shape == D.flat.shape and t._acc_launches == 4
    del calls[:]
    assert _call(t) == ('close', 3)
    assert [c[0] for c in calls] == ['grad_accum', 'adam_step', 'grad_accum', 'adam_step']
    assert calls[0][1][2:] == ('close', A.scale_of(3)) and S.step_lr(calls[1]) == (1, 1e-3) and S.step_lr(calls[3]) == (1, 2e-3)
    assert (t._t_g, t._t_d) == (1, 1) and t._acc_done == 0
    del calls[:]
    # clipping, the weight average and a decay run once per window, on the closed gradient
    t.clip_grad_norm, t.weight_decay = (1.0, None), (1e-2, None)
    monkeypatch.setattr(t, '_clip_ensure', lambda: True), monkeypatch.setattr(t, '_clip_stat', lambda w: 'STAT')
    t._clip = (None, None, None)
    _call(t), _call(t)
    assert [c[0] for c in calls] == ['grad_accum'] * 4
    _call(t)
    assert [c[0] for c in calls[4:]] == ['grad_accum', 'grad_norm', 'adamw_step', 'grad_accum', 'adam_step']
    del calls[:]
    t.clip_grad_norm = t.weight_decay = t._clip = None
    del t._clip_ensure, t._clip_stat          # (the instance's stand-ins: the class's own methods again)
    # a short window: step_accumulated() closes what is there, once
    assert _call(t) == ('begin', 1) and _call(t) == ('add', 2)
    del calls[:]
    assert t.step_accumulated() is True
    assert [c[0] for c in calls] == ['grad_accum', 'adam_step', 'grad_accum', 'adam_step']
    assert calls[0][1][2:] == ('close_only', A.scale_of(2)) and calls[2][1][2:] == ('close_only', A.scale_of(2))
    assert (t._t_g, t._t_d) == (3, 3) and t._acc_done == 0
    del calls[:]
    assert t.step_accumulated() is False and calls == []
    # discards: setup_optimizers(), a change of the window length, switching it off
    _call(t)
    t.setup_optimizers(1e-3, 2e-3)
    assert t._acc_done == 0 and _call(t) == ('begin', 1)
    t.accumulate = 2
    assert _call(t) == ('begin', 1) and _call(t) == ('close', 2)
    _call(t)
    t.accumulate = None
    assert _call(t) is None and t._acc_done == 0
    t.accumulate = 2
    assert _call(t) == ('begin', 1)


def test_kind_key_and_spectral_order(tmp_path, monkeypatch):
    calls = _spied(monkeypatch)
    t = _trainer(tmp_path, spectral=True)
    t.setup_optimizers(1e-3, 1e-3)
    D = t.discriminator
    t.generator.ensure_grad_flat(), D.ensure_grad_flat()
    monkeypatch.setattr(D, 'spectral_grad_map', lambda g: calls.append(('map', (g,), {})))
    t.accumulate = 2
    keys = []
    for want in ('begin', 'close'):
        t._acc_cur = t._acc_begin_call()
        keys.append(t._acc_key())
        assert keys[-1] == (('accum', 2, want),)
        t._adam_step('d')
        t._acc_done = 0 if want == 'close' else 1
    t._acc_cur = None
    # every call maps its own gradient BEFORE it joins the window; the closing call maps once, not again in front of Adam
    assert [c[0] for c in calls] == ['map', 'grad_accum', 'map', 'grad_accum', 'adam_step']
    del calls[:]
    t._acc_cur = t._acc_begin_call()
    t._adam_step('d')
    t._acc_done, t._acc_cur = 1, None
    del calls[:]
    t.step_accumulated()          # the accumulator holds mapped gradients: no map in front of the short close
    assert [c[0] for c in calls] == ['grad_accum', 'adam_step', 'grad_accum', 'adam_step']
    assert t._acc_key() == ()
