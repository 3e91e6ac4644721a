"""Differentiable augmentation (Trainer.diffaug) without a GPU: the NumPy restatement of the map and its adjoint (exact transpose,
equal to torch autograd through the helper's indexing), the augmented oracle trainer against the plain one, the C ABI's argument
validation (before any launch), policy parsing, the YAML keys, and the trainer's plumbing against a recording stand-in."""
import os
import re
import types

import numpy as np
import pytest
import torch
import yaml

from oracle import patchgan_oracle as O
from tests import diffaug_util as U
from tests.golden_util import Golden, LOSS_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pg_diffaug_params', 'pg_diffaug_fwd', 'pg_diffaug_bwd')
SIZES = ((8, 12), (16, 16))


# ---------------------------------------------------------------------------------------------- 1. the restatement
def _int_array(shape, seed):
    return np.random.default_rng(seed).integers(-50, 51, size=shape).astype(np.float64)


def _tables(N, H, W, policy):
    out = [U.masked(t, policy) for t in U.extreme_tables(N, H, W)]
    out += [U.params_ref(seed, t, policy, 0, N, H, W) for seed, t in ((0, 0), (7, 3))]
    return out


@pytest.mark.parametrize('policy', [U.FLIP, U.TRANSLATION, U.CUTOUT, 7], ids=['flip', 'translation', 'cutout', 'all'])
@pytest.mark.parametrize('H,W', SIZES)
def test_adjoint_is_the_exact_transpose(H, W, policy):
    N, C = 5, 3
    x, g = _int_array((N, H, W, C), 1), _int_array((N, H, W, C), 2)
    moved = 0
    for table in _tables(N, H, W, policy):
        a, b = U.apply(x, table), U.adjoint(g, table)
        assert (a * g).sum() == (x * b).sum()              # integers in float64: exact
        # the map moves values or writes +0: the multiset of non-zero outputs is a sub-multiset of the inputs
        assert np.isin(a, np.concatenate([x.ravel(), [0.0]])).all()
        moved += int((a != x).any())
    assert moved >= 3                                       # the tables do something
    # the hand-made tables carry the largest shifts of both signs and boxes over each border
    ext = np.concatenate(U.extreme_tables(N, H, W))
    assert ext[:, 1].max() == H // 8 and ext[:, 1].min() == -(H // 8) and ext[:, 2].max() == W // 8 and ext[:, 2].min() == -(W // 8)
    assert (ext[:, 3] < 0).any() and (ext[:, 3] + ext[:, 5] > H).any() and (ext[:, 4] < 0).any() and (ext[:, 4] + ext[:, 6] > W).any()


def test_neutral_table_is_the_identity_and_each_step_does_what_it_says():
    x = _int_array((1, 8, 12, 2), 3)
    assert np.array_equal(U.apply(x, [U.NEUTRAL_ROW]), x) and np.array_equal(U.adjoint(x, [U.NEUTRAL_ROW]), x)
    assert np.array_equal(U.apply(x, [(1, 0, 0, 0, 0, 0, 0, 0)]), x[:, :, ::-1])
    sh = U.apply(x, [(0, 1, -2, 0, 0, 0, 0, 0)])
    assert np.array_equal(sh[:, 1:, :-2], x[:, :-1, 2:]) and not sh[:, 0].any() and not sh[:, :, -2:].any()
    cut = U.apply(x, [(0, 0, 0, -1, 10, 4, 6, 0)])
    assert not cut[:, :3, 10:].any() and np.array_equal(cut[:, 3:], x[:, 3:]) and np.array_equal(cut[:, :, :10], x[:, :, :10])
    # the order: flip, then translation, then the box (in the augmented frame)
    both = U.apply(x, [(1, 1, -2, 0, 0, 2, 3, 0)])
    want = U.apply(U.apply(U.apply(x, [(1, 0, 0, 0, 0, 0, 0, 0)]), [(0, 1, -2, 0, 0, 0, 0, 0)]), [(0, 0, 0, 0, 0, 2, 3, 0)])
    assert np.array_equal(both, want)


def test_parameter_draw_ranges_neutral_values_and_counter_based_stream():
    H, W = 8, 12
    rows = np.concatenate([U.params_ref(5, t, 7, 0, 16, H, W) for t in range(16)])
    assert set(rows[:, 0]) == {0, 1}
    assert rows[:, 1].min() == -1 and rows[:, 1].max() == 1 and rows[:, 2].min() == -1 and rows[:, 2].max() == 1
    assert rows[:, 3].min() == -2 and rows[:, 3].max() == H - 2 and rows[:, 4].min() == -3 and rows[:, 4].max() == W - 3
    assert (rows[:, 5] == 4).all() and (rows[:, 6] == 6).all() and not rows[:, 7].any()
    for policy in U.POLICIES:
        p = U.params_ref(5, 2, policy, 0, 6, H, W)
        assert np.array_equal(p, U.masked(U.params_ref(5, 2, 7, 0, 6, H, W), policy))          # an off bit: the neutral value, same draws
    whole = U.params_ref(9, 4, 7, 0, 6, 256, 256)
    assert np.array_equal(np.concatenate([U.params_ref(9, 4, 7, 0, 2, 256, 256), U.params_ref(9, 4, 7, 2, 4, 256, 256)]), whole)
    assert not np.array_equal(U.params_ref(9, 5, 7, 0, 6, 256, 256), whole) and not np.array_equal(U.params_ref(8, 4, 7, 0, 6, 256, 256), whole)
    seed = U.find_seed(2, 256, 256)
    assert all(U.interesting(r, 256, 256) for r in U.params_ref(seed, 0, 7, 0, 2, 256, 256))


@pytest.mark.parametrize('H,W', SIZES)
def test_torch_autograd_through_the_map_is_the_adjoint(H, W):
    N, C = 5, 3
    g = np.random.default_rng(4).standard_normal((N, H, W, C)).astype(np.float32)
    xv = np.random.default_rng(5).standard_normal((N, H, W, C)).astype(np.float32)
    for table in _tables(N, H, W, 7):
        x = torch.from_numpy(xv).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        out = U.apply_torch(x, table)
        assert np.array_equal(out.detach().permute(0, 2, 3, 1).numpy(), U.apply(xv, table))
        out.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
        got, want = x.grad.permute(0, 2, 3, 1).contiguous().numpy(), U.adjoint(g, table)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))          # bit for bit


def test_aug_oracle_with_a_neutral_table_is_the_plain_oracle():
    gold = Golden('a_lrelu_tversky')
    c = gold.cfg
    x, y = gold.inputs()
    kw = dict(activation=c['activation'], final_act=c['final_act'], n_layers=c['n_layers'], norm=c['norm'], loss_type=c['loss_type'])
    plain = O.OracleTrainer(gold.weights('g0'), gold.weights('d0'), **kw)
    aug = U.AugOracleTrainer(gold.weights('g0'), gold.weights('d0'), **kw)
    aug.table = np.zeros((x.shape[0], 8), dtype=np.int32)
    for _ in range(2):
        a, b = plain.batch(x, y, train=True), aug.batch(x, y, train=True)
        assert [a[k] for k in LOSS_KEYS] == [b[k] for k in LOSS_KEYS]
    for k in plain.gw:
        assert torch.equal(plain.gw[k], aug.gw[k]), k
    for k in plain.dw:
        assert torch.equal(plain.dw[k], aug.dw[k]), k
    # ... and a table that does something moves the curve (the helper's D really reads the map)
    aug.table = U.params_ref(U.find_seed(x.shape[0], 256, 256), 0, 7, 0, x.shape[0], 256, 256)
    assert plain.batch(x, y, train=True)['gdisc'] != aug.batch(x, y, train=True)['gdisc']


# ---------------------------------------------------------------------------------------------- 2. C ABI
def test_new_symbols_declared_exported_bound_and_validated_before_any_launch():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    m = {k: int(v) for k, v in re.findall(r'#define (PG_AUG_[A-Z]+) (\d+)', src)}
    assert m == {'PG_AUG_FLIP': 1, 'PG_AUG_TRANSLATION': 2, 'PG_AUG_CUTOUT': 4}
    assert (_lib.AUG_FLIP, _lib.AUG_TRANSLATION, _lib.AUG_CUTOUT) == (U.FLIP, U.TRANSLATION, U.CUTOUT) == (1, 2, 4)
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    a = 1 << 20           # non-NULL aligned addresses that are never dereferenced: every call below is refused on the host
    b = 1 << 24
    assert lib.pg_diffaug_params(0, a, 0, 7, 0, 2, 8, 8, None, None) == -1
    assert lib.pg_diffaug_params(0, a + 4, 0, 7, 0, 2, 8, 8, b, None) == -1          # misaligned counter
    assert lib.pg_diffaug_params(0, a, 0, 7, 0, 2, 8, 8, b + 2, None) == -1          # misaligned table
    for bad in ((8, 0, 2, 8, 8), (-1, 0, 2, 8, 8), (7, -1, 2, 8, 8), (7, 0, 0, 8, 8), (7, 0, 2, 0, 8), (7, 0, 2, 8, -3)):
        assert lib.pg_diffaug_params(0, a, 0, *bad, b, None) == -1, bad
    for fn in (lib.pg_diffaug_fwd, lib.pg_diffaug_bwd):
        good = [a, 4, b, 4, a, 2, 8, 8, 4, None]
        for i in (0, 2, 4):                                  # src, dst, table: each NULL on its own
            args = list(good)
            args[i] = None
            assert fn(*args) == -1, i
        assert fn(a, 3, b, 4, a, 2, 8, 8, 4, None) == -1 and fn(a, 4, b, 3, a, 2, 8, 8, 4, None) == -1          # ld < C
        for i in (5, 6, 7, 8):
            args = list(good)
            args[i] = 0
            assert fn(*args) == -1, i
        assert fn(a, 4, a, 4, b, 2, 8, 8, 4, None) == -1                                                          # the same buffer
        assert fn(a, 8, a + 16, 8, b, 2, 8, 8, 4, None) == -1                                                     # interleaved slices of one
        n_bytes = 2 * 8 * 8 * 4 * 4
        assert fn(a, 4, a + n_bytes - 4, 4, b, 2, 8, 8, 4, None) == -1                                            # one element shared
        assert fn(a, 4, b, 4, a, 1 << 16, 1 << 8, 1 << 7, 4, None) == -1                                          # N*H*W = 2^31


# ---------------------------------------------------------------------------------------------- 3. the setting
def test_policy_parser():
    from patchgan_amd import engine as E
    assert E.diffaug_policy(None) == 0 and E.diffaug_policy('') == 0 and E.diffaug_policy([]) == 0 and E.diffaug_policy(()) == 0
    assert E.diffaug_policy('flip') == 1 and E.diffaug_policy('translation') == 2 and E.diffaug_policy('cutout') == 4
    assert E.diffaug_policy('cutout,flip') == 5 and E.diffaug_policy(' translation , cutout ') == 6
    assert E.diffaug_policy(['flip', 'translation', 'cutout']) == 7 and E.diffaug_policy(('cutout', 'cutout')) == 4
    for names in U.subsets():
        assert E.diffaug_policy(','.join(names)) == E.diffaug_policy(list(names)) == sum(U.NAMES[n] for n in names)
    for bad in ('color', 'flip,colour', 'Flip', ['flip', 3], 7, True, {'flip': 1}, 'flip translation', ['flip,cutout']):
        with pytest.raises(ValueError, match='flip, translation, cutout'):
            E.diffaug_policy(bad)
    assert E.diffaug_seed(0) == 0 and E.diffaug_seed(2 ** 64 - 1) == 2 ** 64 - 1 and E.diffaug_seed(np.int64(5)) == 5
    for bad in (-1, 2 ** 64, 1.5, '3', None, True):
        with pytest.raises(ValueError):
            E.diffaug_seed(bad)


TRAIN_YAML = """
train_params:
  loss_type: weighted_bce
  seg_alpha: 100
  gen_learning_rate: 1.e-3
  disc_learning_rate: 1.e-3
%s
"""


def _trainer(tmp_path, seed=3):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, 1, 4, use_dropout=False, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    return pg.Trainer(g, d, str(tmp_path))


def test_yaml_keys_reach_the_trainer(tmp_path):
    import patchgan_amd as pg
    from patchgan_amd.train import apply_train_params
    assert pg.Trainer.diffaug is None and pg.Trainer.diffaug_seed == 0
    t = _trainer(tmp_path)
    for text, want, seed in (('', None, 0), ('  diffaug: translation,cutout', 'translation,cutout', 0),
                             ('  diffaug: [flip, cutout]\n  diffaug_seed: 11', ['flip', 'cutout'], 11),
                             ('  diffaug: ""', None, 0), ('  diffaug: []', None, 0), ('  diffaug_seed: 4', None, 4)):
        apply_train_params(t, yaml.safe_load(TRAIN_YAML % text)['train_params'])
        assert t.diffaug == want and t.diffaug_seed == seed and t.loss_type == 'weighted_bce', text
        assert t._aug_now() == (None if want is None else (sum(U.NAMES[n] for n in (want.split(',') if isinstance(want, str) else want)), seed))
    for text in ('  diffaug: color', '  diffaug: [flip, 3]', '  diffaug: 7', '  diffaug: true', '  diffaug: {flip: 1}',
                 '  diffaug: flip\n  diffaug_seed: -1', '  diffaug: flip\n  diffaug_seed: 1.5', '  diffaug_seed: abc'):
        with pytest.raises(ValueError):
            apply_train_params(t, yaml.safe_load(TRAIN_YAML % text)['train_params'])
    import patchgan
    assert patchgan.Trainer.diffaug is None and hasattr(patchgan.Trainer, 'read_diffaug_params')


def test_kind_key_gains_policy_and_seed_only_when_on(tmp_path):
    t = _trainer(tmp_path)
    t.setup_optimizers()
    x = torch.zeros(2, 3, 256, 256)
    args = (x, x[:, :1], False, (2, 256, 256, 3, 1))
    off = t._kind_key(*args, True)
    assert off == t._kind_key_base(*args, True) and t._aug_counter is None
    for empty in ('', [], ()):
        t.diffaug = empty
        assert t._kind_key(*args, True) == off and t._aug_now() is None
    keys = {off}
    for policy, seed in (('flip', 0), ('flip', 1), ('cutout', 0), ('flip,cutout', 0), (['translation'], 0)):
        t.diffaug, t.diffaug_seed = policy, seed
        k = t._kind_key(*args, True)
        assert k[:len(off)] == off and k not in keys
        keys.add(k)
        assert t._kind_key(*args, False) == t._kind_key_base(*args, False)          # an evaluation step never augments
    t.diffaug, t.diffaug_seed = 'cutout , flip', 0
    assert t._kind_key(*args, True) in keys                                         # the same bits: the same kind
    t.diffaug = 'colour'
    with pytest.raises(ValueError):
        t._kind_key(*args, True)
    t.diffaug = None
    with pytest.raises(RuntimeError):
        t.read_diffaug_params()


# ---------------------------------------------------------------------------------------------- 4. the trainer's plumbing
class _Ctx:
    """What a discriminator pass returns, as far as the step looks at it."""

    def __init__(self, E, din, n=None):
        self.din = din
        self.out = E.View.alloc(din.N if n is None else n, 2, 2, 1, torch.device('cpu'))

    def samples(self, n0, n):
        c = _Ctx.__new__(_Ctx)
        c.din, c.out = self.din, self.out.samples(n0, n)
        return c


class _Spy:
    """Stands in for patchgan_amd.engine inside the trainer module: records the entry points a step reaches, launches nothing."""
    RECORDED = ('din_fill', 'loss_begin', 'loss_finish', 'loss_value_and_grad', 'side_join', 'seg_confusion')

    def __init__(self, real, log, two):
        self._real, self.log = real, log
        self.ex = types.SimpleNamespace(enabled=two, pending=False, keep=[], device=torch.device('cpu'))

    def cur_exec(self, device=None):
        return self.ex

    def on_side(self):
        spy = self

        class Fork:
            def __enter__(self):
                spy.log.append(('fork',))

            def __exit__(self, *exc):
                spy.log.append(('fork_end',))
                return False
        return Fork()

    def diffaug_params(self, seed, counter, step, policy, sample0, N, H, W):
        self.log.append(('diffaug_params', seed, counter, step, policy, sample0, N, H, W))
        return torch.zeros(N, 8, dtype=torch.int32)

    def diffaug_fwd(self, src, dst, params, n0=0):
        self.log.append(('diffaug_fwd', src, dst, params, n0))
        return dst

    def diffaug_bwd(self, g, dsrc, params, n0=0):
        self.log.append(('diffaug_bwd', g, dsrc, params, n0))
        return dsrc

    def __getattr__(self, name):
        if name in self.RECORDED:
            return lambda *a, **k: self.log.append((name,) + a)
        return getattr(self._real, name)


def _step(monkeypatch, tmp_path, train, two, halves, **attrs):
    """One Trainer._enqueue_step on CPU tensors with every launch replaced by a record.  -> (trainer, log)."""
    from patchgan_amd import trainer as T
    t = _trainer(tmp_path)
    for k, v in attrs.items():
        setattr(t, k, v)
    t.setup_optimizers()
    log = []
    spy = _Spy(T.E, log, two)
    monkeypatch.setattr(T, 'E', spy)
    monkeypatch.setattr(t, '_adam_step', lambda which: log.append(('adam', which)))
    N, H, W, Cin, Cout = 2, 16, 16, 3, 1
    G, D = t.generator, t.discriminator
    ge, de = G.engine, D.engine
    cpu = torch.device('cpu')
    monkeypatch.setattr(ge, 'ucache_begin', lambda *a, **k: {})
    monkeypatch.setattr(ge, 'ucache_end', lambda *a, **k: None)
    monkeypatch.setattr(ge, 'forward', lambda *a, **k: log.append(('ge.forward',) + a) or 'gc')
    monkeypatch.setattr(ge, 'backward', lambda *a, **k: log.append(('ge.backward',) + a))
    monkeypatch.setattr(de, 'ucache_begin', lambda *a, **k: {})
    monkeypatch.setattr(de, 'ucache_end', lambda *a, **k: None)
    monkeypatch.setattr(de, 'halves_ok', lambda *a: halves)
    monkeypatch.setattr(de, 'context', lambda flat, din, **k: log.append(('de.context', din)) or _Ctx(spy, din))
    monkeypatch.setattr(de, 'forward_part', lambda flat, c, n0, n, **k: log.append(('de.forward_part', c.din, n0, n)))
    monkeypatch.setattr(de, 'forward', lambda flat, din, **k: log.append(('de.forward', din)) or _Ctx(spy, din))

    def d_backward(flat, gflat, c, gout, need_wgrad=True, need_dx=False, ucache=None):
        log.append(('de.backward', c.din, need_wgrad, need_dx))
        return spy.View.alloc(N, H, W, Cin + Cout, cpu) if need_dx else None
    monkeypatch.setattr(de, 'backward', d_backward)
    if train and t.diffaug is not None:
        t._aug_ensure()
    x, y = torch.zeros(N, Cin, H, W), torch.zeros(N, Cout, H, W)
    t._enqueue_step(x, y, False, N, H, W, Cin, Cout, train)
    t._deferred = None
    return t, log


def _names(log):
    return [r[0] for r in log]


@pytest.mark.parametrize('halves', [False, True], ids=['three_passes', 'shared_halves'])
@pytest.mark.parametrize('two', [False, True], ids=['one_stream', 'two_streams'])
def test_off_issues_no_diffaug_call_and_on_orders_them(monkeypatch, tmp_path, two, halves):
    t_off, off = _step(monkeypatch, tmp_path / 'a', True, two, halves)
    assert not any(n.startswith('diffaug') for n in _names(off)) and t_off._aug_counter is None and t_off._aug_params is None
    t_none, none = _step(monkeypatch, tmp_path / 'b', True, two, halves, diffaug=None)
    assert _names(none) == _names(off)
    t, on = _step(monkeypatch, tmp_path / 'c', True, two, halves, diffaug='translation,cutout', diffaug_seed=9)
    names = _names(on)
    # the same step plus exactly four launches: one table, the two halves' moves, the adjoint
    assert [n for n in names if not n.startswith('diffaug')] == _names(off)
    assert [n for n in names if n.startswith('diffaug')] == ['diffaug_params', 'diffaug_fwd', 'diffaug_fwd', 'diffaug_bwd']
    par = on[names.index('diffaug_params')]
    assert par[1] == 9 and par[2] is t._aug_counter and par[4] == 6 and par[5:] == (0, 2, 16, 16)          # seed, counter, bits, sample0, N, H, W
    assert t._aug_counter.dtype == torch.int64 and t._aug_counter.numel() == 1
    fwd = [r for r in on if r[0] == 'diffaug_fwd']
    table = fwd[0][3]
    assert t._aug_params is table and fwd[1][3] is table and fwd[0][4] == fwd[1][4] == 0          # paired: the same rows for both halves
    (real, real_d), (fake, fake_d) = fwd[0][1:3], fwd[1][1:3]
    din_t, aug_t = real.t, real_d.t
    assert fake.t is din_t and fake_d.t is aug_t and aug_t is not din_t and aug_t.numel() == din_t.numel()
    assert (real.off, fake.off) == (real_d.off, fake_d.off) and real.ld == real_d.ld and (real.N, real.C) == (2, 4) == (fake_d.N, fake_d.C)
    # the table and the real half ahead of the generator forward and of the fork; the fake half right behind the generator forward
    i_gen = names.index('ge.forward')
    assert names.index('diffaug_params') < names.index('diffaug_fwd') < i_gen and names[i_gen + 1] == 'diffaug_fwd'
    if two:
        assert names.index('diffaug_fwd') < names.index('fork') and i_gen + 1 < names.index('fork')
    # the generator and its loss stay on the un-augmented buffer; every D pass reads the augmented one
    assert on[i_gen][2].t is din_t and on[i_gen][3].t is din_t
    assert on[names.index('loss_begin')][1].t is din_t
    d_reads = [r[1] for r in on if r[0] in ('de.context', 'de.forward', 'de.forward_part', 'de.backward')]
    assert len(d_reads) >= 4 and all(v.t is aug_t for v in d_reads)
    off_din_t = off[_names(off).index('din_fill')][3].t
    assert all(r[1].t is off_din_t for r in off if r[0] in ('de.context', 'de.forward', 'de.forward_part', 'de.backward'))
    assert on[names.index('din_fill')][3].t is din_t
    # the gradient returns through the adjoint into a fresh [N, H, W, Cout] view, and that view is what G's backward receives
    bwd = on[names.index('diffaug_bwd')]
    assert names.index('de.backward') < names.index('diffaug_bwd') < names.index('ge.backward')
    assert (bwd[1].off, bwd[1].C, bwd[1].ld) == (3, 1, 4) and (bwd[2].off, bwd[2].C, bwd[2].ld, bwd[2].N) == (0, 1, 1, 2) and bwd[3] is table
    assert on[names.index('ge.backward')][5] is bwd[2]
    g2_off = off[_names(off).index('ge.backward')][5]
    assert (g2_off.off, g2_off.C, g2_off.ld) == (3, 1, 4)


def test_evaluation_steps_never_augment(monkeypatch, tmp_path):
    t, log = _step(monkeypatch, tmp_path, False, False, False, diffaug='flip,translation,cutout')
    assert not any(n.startswith('diffaug') for n in _names(log)) and t._aug_params is None
    assert 'ge.backward' not in _names(log) and 'adam' not in _names(log)
