"""Gradient-norm clipping (Trainer.clip_grad_norm) without a GPU: the C ABI of pg_grad_norm / pg_adam_clip_step / pg_adam_clip_step_dev
(argument validation happens before any launch), engine.check_clip_norm, the trainer's dispatch and step key, the YAML key, and the
comparator of tests/gradclip_util.py: the plain fp32 emulation passes every case and every mutation is rejected by the named check."""
import math
import os
import re

import pytest
import torch
import yaml

from tests import adam_spy as S
from tests import gradclip_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pg_grad_norm_workspace_bytes', 'pg_grad_norm', 'pg_adam_clip_step', 'pg_adam_clip_step_dev')
INF = float('inf')


def _trainer(tmp_path, clip=None, seed=3):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid')
    d = pg.Discriminator(4, 4, n_layers=3)
    t = pg.Trainer(g, d, str(tmp_path))
    if clip is not None:
        t.clip_grad_norm = clip
    return t


# ---------------------------------------------------------------------------------------------- 1. C ABI
def test_new_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib, engine as E
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # the plain forms' arguments, plus the ema pointer, the decay and the status block
    assert len(_lib.SIGNATURES['pg_adam_clip_step'][1]) == len(_lib.SIGNATURES['pg_adam_step'][1]) + 3
    assert len(_lib.SIGNATURES['pg_adam_clip_step_dev'][1]) == len(_lib.SIGNATURES['pg_adam_step_dev'][1]) + 3
    # the status block: the header's struct, the engine's record and the tests' are one layout
    m = re.search(r'typedef struct pg_grad_stat \{(.*?)\} pg_grad_stat;', src, flags=re.S)
    names = [x.strip().split(' ')[-1] for decl in m.group(1).split(';') if decl.strip() for x in decl.strip().split(',')]
    assert tuple(names) == E.GRAD_STAT.names == U.STAT.names, names
    assert E.GRAD_STAT == U.STAT and E.GRAD_STAT.itemsize == 64


def test_workspace_query_mirrors_the_partition():
    from patchgan_amd import _lib
    lib = _lib.load()
    assert lib.pg_grad_norm_workspace_bytes(0) == 0 and lib.pg_grad_norm_workspace_bytes(-5) == 0
    for n in U.NORM_NS + (U.ADAM_BIG_N, 1 << 33):
        assert lib.pg_grad_norm_workspace_bytes(n) == 8 * U.norm_blocks(n), n
    assert U.norm_blocks(U.CHUNK) == 1 and U.norm_blocks(U.CHUNK + 4) == 2 and U.norm_blocks(U.CHUNK + 3) == 1
    assert U.norm_blocks(U.TRIP) == U.NORM_MAX_BLOCKS == U.norm_blocks(U.TRIP + 4) and U.norm_blocks(U.TRIP - U.CHUNK) == U.NORM_MAX_BLOCKS - 1


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host
    ws = lib.pg_grad_norm_workspace_bytes(4099)
    for i in (0, 3, 5):                                  # g, ws, stat: each NULL on its own
        args = [a, 4099, 1.0, a, ws, a, None]
        args[i] = None
        assert lib.pg_grad_norm(*args) == -1, i
    for bad in (0.0, -1.0, float('nan'), -INF):
        assert lib.pg_grad_norm(a, 4099, bad, a, ws, a, None) == -1, bad
    for n in (0, -4):
        assert lib.pg_grad_norm(a, n, 1.0, a, ws, a, None) == -1
    assert lib.pg_grad_norm(a, 4099, 1.0, a, ws - 1, a, None) == -1          # workspace smaller than the query reports
    assert lib.pg_grad_norm(a, U.TRIP, 1.0, a, ws, a, None) == -1
    assert lib.pg_grad_norm(a + 4, 4099, 1.0, a, ws, a, None) == -1          # misaligned g, stat, ws
    assert lib.pg_grad_norm(a, 4099, 1.0, a, ws, a + 8, None) == -1
    assert lib.pg_grad_norm(a, 4099, 1.0, a + 4, ws, a, None) == -1
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.999)
    tail_dev = (0.9, 0.999, 1e-8, a, 0.999)
    for i in (0, 1, 2, 3):                               # p, g, m, v: each NULL on its own (a NULL ema is the form without the average)
        ptrs = [a] * 5
        ptrs[i] = None
        assert lib.pg_adam_clip_step(*ptrs, 10, *tail, a, None) == -1, i
        assert lib.pg_adam_clip_step_dev(*ptrs, 10, *tail_dev, a, None) == -1, i
    for ema in (a, None):
        assert lib.pg_adam_clip_step(a, a, a, a, ema, 10, *tail, None, None) == -1          # stat
        assert lib.pg_adam_clip_step_dev(a, a, a, a, ema, 10, *tail_dev, None, None) == -1
        assert lib.pg_adam_clip_step_dev(a, a, a, a, ema, 10, 0.9, 0.999, 1e-8, None, 0.999, a, None) == -1      # scalars
        assert lib.pg_adam_clip_step(a, a, a, a, ema, 10, *tail, a + 8, None) == -1         # misaligned stat
        assert lib.pg_adam_clip_step(a, a + 4, a, a, ema, 10, *tail, a, None) == -1         # misaligned g
        for n in (0, -4):
            assert lib.pg_adam_clip_step(a, a, a, a, ema, n, *tail, a, None) == -1
            assert lib.pg_adam_clip_step_dev(a, a, a, a, ema, n, *tail_dev, a, None) == -1
    for decay in (1.0, -0.1, float('nan')):              # read only with an ema pointer
        assert lib.pg_adam_clip_step(a, a, a, a, a, 10, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, decay, a, None) == -1, decay
        assert lib.pg_adam_clip_step_dev(a, a, a, a, a, 10, 0.9, 0.999, 1e-8, a, decay, a, None) == -1, decay
    assert lib.pg_adam_clip_step(a, a, a, a, a + 4, 10, *tail, a, None) == -1               # misaligned ema


# ---------------------------------------------------------------------------------------------- 2. the setting
def test_check_clip_norm():
    from patchgan_amd import engine as E
    import numpy as np
    assert E.check_clip_norm(None) == (None, None)
    assert E.check_clip_norm(2) == (2.0, 2.0) and E.check_clip_norm(0.5) == (0.5, 0.5) and E.check_clip_norm(np.float32(4)) == (4.0, 4.0)
    assert E.check_clip_norm(INF) == (INF, INF)
    assert E.check_clip_norm((1.0, None)) == (1.0, None) and E.check_clip_norm([None, 3]) == (None, 3.0)
    assert E.check_clip_norm((None, None)) == (None, None) and E.check_clip_norm((INF, 2.5)) == (INF, 2.5)
    for bad in (True, False, 0, 0.0, -1.0, float('nan'), -INF, 'x', '1.0', (1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), (True, 1.0), (1.0, 'x'),
                {'gen': 1.0}, (float('nan'), None)):
        with pytest.raises(ValueError):
            E.check_clip_norm(bad)


@pytest.mark.parametrize('bad', [0.0, -1.0, float('nan'), True, 'x', (1.0,)], ids=['zero', 'negative', 'nan', 'bool', 'string', 'one_tuple'])
def test_bad_setting_raises_value_error(tmp_path, bad):
    t = _trainer(tmp_path, bad)
    with pytest.raises(ValueError):
        t.setup_optimizers()
    t2 = _trainer(tmp_path)
    t2.setup_optimizers()
    t2.clip_grad_norm = bad
    with pytest.raises(ValueError):
        t2._adam_step('g')
    x = torch.zeros(2, 3, 256, 256)
    with pytest.raises(ValueError):
        t2._kind_key(x, x[:, :1], False, (2, 256, 256, 3, 1), True)


def _dispatch(monkeypatch, t, dev):
    """The entry points _adam_step reaches for both networks (adam_spy: recorded at engine.adam_update, nothing is launched)."""
    calls = S.spy(monkeypatch)
    t._adam_dev = torch.zeros(4) if dev else None
    t._adam_step('g')
    t._adam_step('d')
    t._adam_dev = None
    return calls


@pytest.mark.parametrize('dev', [False, True], ids=['args', 'dev_scalars'])
@pytest.mark.parametrize('decay', [None, 0.99], ids=['plain', 'ema'])
def test_default_none_reaches_only_the_existing_entry_points(tmp_path, monkeypatch, decay, dev):
    import patchgan_amd as pg
    assert pg.Trainer.clip_grad_norm is None
    t = _trainer(tmp_path)
    t.ema_decay = decay
    t.setup_optimizers()
    assert t._clip is None and t._clip_now() == (None, None)
    names = [c[0] for c in _dispatch(monkeypatch, t, dev)]
    g_name = ('adam_ema_step' if decay else 'adam_step') + ('_dev' if dev else '')
    assert names == [g_name, 'adam_step' + ('_dev' if dev else '')]
    assert t._clip is None                      # no buffer either
    with pytest.raises(RuntimeError):
        t.read_grad_stats()
    with pytest.raises(RuntimeError):
        t.reset_grad_stats()
    t.clip_grad_norm = (None, None)             # a pair of Nones is off as well
    assert [c[0] for c in _dispatch(monkeypatch, t, dev)] == names and t._clip is None
    with pytest.raises(RuntimeError):
        t.read_grad_stats()


@pytest.mark.parametrize('dev', [False, True], ids=['args', 'dev_scalars'])
@pytest.mark.parametrize('decay', [None, 0.99], ids=['plain', 'ema'])
@pytest.mark.parametrize('clip', [2.0, INF, (1.5, None), (None, 0.5)], ids=['both', 'monitor', 'gen_only', 'disc_only'])
def test_a_value_puts_the_norm_in_front_of_the_clipped_adam(tmp_path, monkeypatch, clip, decay, dev):
    from patchgan_amd import engine as E
    t = _trainer(tmp_path, clip)
    t.ema_decay = decay
    t.setup_optimizers()
    stat, ws_g, ws_d = t._clip
    assert stat.dtype == torch.float64 and stat.numel() * 8 == 2 * E.GRAD_STAT.itemsize and not bool(stat.any())
    assert ws_g.numel() * 8 >= E.grad_norm_workspace_bytes(t.generator.flat.numel()) and ws_g.data_ptr() != ws_d.data_ptr()
    assert t._clip_stat('d').data_ptr() == t._clip_stat('g').data_ptr() + 64
    t0 = (t._t_g, t._t_d)
    calls = _dispatch(monkeypatch, t, dev)
    gmax, dmax = E.check_clip_norm(clip)
    want = []
    for which, mx, net, ws in (('g', gmax, t.generator, ws_g), ('d', dmax, t.discriminator, ws_d)):
        ema = decay is not None and which == 'g'
        if mx is None:
            want.append(('adam_ema_step' if ema else 'adam_step') + ('_dev' if dev else ''))
            continue
        want += ['grad_norm', 'adam_clip_step' + ('_dev' if dev else '')]
        norm, step = calls[len(want) - 2], calls[len(want) - 1]
        assert norm[1][0] is net.grad_flat and norm[1][1] == mx and norm[1][2] is ws
        assert norm[1][3].data_ptr() == t._clip_stat(which).data_ptr()
        assert step[1][0] is net.flat and step[1][1] is net.grad_flat
        assert (step[2]['ema'] is t._ema) if ema else (step[2]['ema'] is None)          # the average rides along for G only
        assert step[2]['ema_decay'] == (decay if ema else None)
        assert step[2]['stat'].data_ptr() == t._clip_stat(which).data_ptr()
    assert [c[0] for c in calls] == want
    # the host's step counts advance as without the feature (a captured step's are advanced by the replay)
    assert (t._t_g, t._t_d) == ((t0[0], t0[1]) if dev else (t0[0] + 1, t0[1] + 1))


def test_kind_key_and_graph_pointers(tmp_path):
    t = _trainer(tmp_path)
    t.ema_decay = 0.9
    t.setup_optimizers()
    x = torch.zeros(2, 3, 256, 256)
    args = (x, x[:, :1], False, (2, 256, 256, 3, 1))
    off = t._kind_key(*args, True)
    assert off == t._kind_key_base(*args, True) and len(off) == 23           # the key of the tree without the feature
    assert t._graph_ptrs()[-1] == t._ema.data_ptr() and t._graph_ptrs()[-4:-1] == (0, 0, 0)
    keys = {off}
    for clip in (1.0, 2.0, INF, (1.0, None), (None, 1.0), (1.0, 2.0)):
        t.clip_grad_norm = clip
        k = t._kind_key(*args, True)
        assert k[:len(off)] == off and k not in keys, clip
        keys.add(k)
        assert t._kind_key(*args, False) == t._kind_key_base(*args, False)      # an evaluation step launches no Adam
    t.clip_grad_norm = (None, None)
    assert t._kind_key(*args, True) == off
    t.clip_grad_norm = 1.0
    t.setup_optimizers()
    ptrs = t._graph_ptrs()
    assert ptrs[-4:-1] == tuple(b.data_ptr() for b in t._clip) and ptrs[-1] == t._ema.data_ptr()
    # persistent: a second setup_optimizers() keeps the buffers and clears the accumulators
    t._clip[0].fill_(1.0)
    t.setup_optimizers()
    assert t._graph_ptrs()[-4:] == ptrs[-4:] and not bool(t._clip[0].any())


def test_read_and_reset_grad_stats_decode_the_status_blocks(tmp_path):
    import numpy as np
    t = _trainer(tmp_path, 1.0)
    t.setup_optimizers()
    rec = np.zeros(2, dtype=U.STAT)
    rec[0] = (3.0, 1.0 / 3.0, 1, 0, 5, 2, 1, 7.5, 16.0, 9.0)
    rec[1] = (float('nan'), 0.0, 0, 0, 2, 0, 2, 0.0, 0.0, float('nan'))
    t._clip[0].copy_(torch.from_numpy(rec.view(np.float64).copy()))
    s = t.read_grad_stats()
    assert s['gen'] == dict(norm=3.0, coef=float(np.float32(1.0 / 3.0)), steps=5, clipped=2, skipped=1, max_norm=7.5, mean_norm=4.0)
    d = s['disc']
    assert math.isnan(d['norm']) and math.isnan(d['mean_norm']) and (d['steps'], d['skipped'], d['coef']) == (2, 2, 0.0)
    t.reset_grad_stats()
    z = t.read_grad_stats()
    assert z['gen']['steps'] == 0 and z['gen']['max_norm'] == 0.0 and math.isnan(z['gen']['mean_norm'])
    assert t.grad_history == []


# ---------------------------------------------------------------------------------------------- 3. YAML
TRAIN_YAML = """
train_params:
  loss_type: weighted_bce
  seg_alpha: 100
  gen_learning_rate: 1.e-3
  disc_learning_rate: 1.e-3
  clip_grad_norm: %s
"""


def test_yaml_key_reaches_the_trainer(tmp_path):
    from patchgan_amd.train import apply_train_params
    from patchgan_amd import engine as E
    t = _trainer(tmp_path)
    cfg = yaml.safe_load(TRAIN_YAML % '5.0')
    apply_train_params(t, cfg['train_params'])
    assert t.clip_grad_norm == 5.0 and t.loss_type == 'weighted_bce' and t.seg_alpha == 100
    assert t._clip_now() == (5.0, 5.0)
    for text, want in (('[10.0, 2.5]', (10.0, 2.5)), ('[null, 1]', (None, 1.0)), ('[.inf, null]', (INF, None)), ('.inf', (INF, INF))):
        cfg = yaml.safe_load(TRAIN_YAML % text)
        apply_train_params(t, cfg['train_params'])
        assert E.check_clip_norm(t.clip_grad_norm) == want == t._clip_now(), text
    del cfg['train_params']['clip_grad_norm']                    # absent = off
    t = _trainer(tmp_path, 0.5)
    apply_train_params(t, cfg['train_params'])
    assert t.clip_grad_norm is None
    # the reference-named package is the same module
    import patchgan
    assert patchgan.Trainer.clip_grad_norm is None and hasattr(patchgan.Trainer, 'read_grad_stats')


# ---------------------------------------------------------------------------------------------- 4. the comparator
def _ratios(case, mut=None, ema=False):
    state, sc, mx = U.case_state(case)
    e = state[0] * 0.5 + 0.25 if ema else None
    c = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.999, dtype=torch.float32)) if ema else None
    return U.clip_ratios(U.plain_clip(state, sc, mx, mut, e, c), state, sc, mx, e, c)


@pytest.mark.parametrize('n', U.NORM_NS, ids=lambda n: f'n{n}')
def test_plain_emulation_passes_every_case(n):
    cases = [c for c in U.clip_cases() if c.n == n]
    assert cases
    for case in cases:
        for ema in (False, True):
            r = _ratios(case, ema=ema)
            assert set(r) >= {'skip', 'sumsq', 'norm', 'coef', 'p', 'm', 'v'} and max(r.values()) <= 1.0, (case, r)
            _, _, mx = U.case_state(case)
            state = U.clip_inputs(case.n, case.kind)
            got = U.plain_clip(state, U.adam_scalars(*U.T_LR), mx)
            clips = case.clip == 'below' and U.norm_ref(state[1]) > 0.0
            assert (got['coef'] < 1.0) == clips and (clips or got['coef'] == 1.0), case


def test_plain_emulation_passes_the_multitrip_case():
    r = _ratios(U.BIG_CASE)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('poison', U.POISONS, ids=lambda p: f'{p[0]}-{p[1]}')
def test_plain_emulation_skips_a_poisoned_step(poison):
    for ema in (False, True):
        r = _ratios((U.ClipCase(U.POISON_N, 'unit', 'below'),) + poison, ema=ema)
        assert r == {'skip': 0.0}, r


def test_huge_gradients_have_a_float_norm_and_an_infinite_fp32_sum():
    import numpy as np
    _, g, _, _ = U.clip_inputs(4099, 'huge')
    assert math.isfinite(float(np.float32(U.norm_ref(g)))) and U.norm_ref(g) >= 1e20 * math.sqrt(4099)
    gf = g.float().numpy()
    with np.errstate(over='ignore'):
        assert np.isinf(np.sum(gf * gf, dtype=np.float32))


@pytest.mark.parametrize('mut', U.NORM_MUTATIONS + U.ADAM_MUTATIONS)
def test_mutation_is_rejected_by_the_named_check(mut):
    case, key = U.clip_mutation_table()[mut]
    clean, bad = _ratios(case), _ratios(case, mut)
    assert max(clean.values()) <= 1.0, clean
    assert bad[key] > 1.0, (mut, key, bad)


def test_every_mutation_has_a_case():
    assert set(U.clip_mutation_table()) == set(U.NORM_MUTATIONS + U.ADAM_MUTATIONS)
    assert len(set(U.NORM_MUTATIONS + U.ADAM_MUTATIONS)) == 13


def test_reference_is_torchs_clip_grad_norm_then_adam():
    """clip_grad_norm_ + torch.optim.Adam on float64 copies of the fp32 state against norm_ref / coef_ref / adam_ref on the scaled
    gradient (float64 throughout, so the product g * coef is not rounded to fp32 here: agreement to 1e-12 relative)."""
    state, sc, mx = U.case_state(U.ClipCase(1023, 'unit', 'below'))
    p, g, m, v = state
    t, lr = U.T_LR
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([q], mx)
    assert abs(float(total) - U.norm_ref(g)) <= 1e-12 * U.norm_ref(g)
    c = U.coef_ref(U.norm_ref(g), mx)
    assert torch.allclose(q.grad, g * c, rtol=1e-12, atol=0)
    opt = torch.optim.Adam([q], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    opt.step()
    (p1, m1, v1), _ = U.adam_ref((p, g * c, m, v), sc)
    # (adam_ref takes beta1, beta2, lr / bc1, sqrt(bc2) as the float32 values the kernel receives: 1e-6 relative to the update)
    gc = g * c
    assert bool(((opt.state[q]['exp_avg'] - m1).abs() <= 1e-6 * (m.abs() + gc.abs())).all())
    assert bool(((opt.state[q]['exp_avg_sq'] - v1).abs() <= 1e-6 * (v + gc * gc)).all())
    assert float(((q.detach() - p) - (p1 - p)).abs().max()) <= 1e-5 * float((p1 - p).abs().max())
