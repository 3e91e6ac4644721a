"""The optimizer's options (Trainer.betas / weight_decay / save_optimizer) without a GPU: the comparator of tests/optim_util.py (the
plain fp32 emulation passes every case, every mutation is rejected at its planted case), the C ABI of pg_adamw_step /
pg_adamw_step_dev (argument validation happens before any launch), engine.check_betas / check_weight_decay, the YAML forms, the
trainer's dispatch and step key, and the layout of the optimizer file against torch.optim.Adam / AdamW."""
import functools
import os
import re

import pytest
import torch
import yaml
from torch import nn

from tests import adam_spy as S
from tests import optim_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pg_adamw_step', 'pg_adamw_step_dev')
NAN, INF = float('nan'), float('inf')


def _nets(spectral=False, affine=False, seed=3):
    import patchgan_amd as pg
    torch.manual_seed(seed)
    kw = dict(norm_layer=functools.partial(nn.InstanceNorm2d, affine=True)) if affine else {}
    g = pg.UNet(3, 1, 4, activation='leakyrelu', final_act='sigmoid', **kw)
    d = pg.Discriminator(4, 4, n_layers=3, norm=affine, spectral_norm=spectral, **kw)
    return g, d


def _trainer(tmp_path, **kw):
    import patchgan_amd as pg
    g, d = _nets(**kw)
    return pg.Trainer(g, d, str(tmp_path))


# ---------------------------------------------------------------------------------------------- 1. soundness of the bound
@pytest.mark.parametrize('n', U.ADAM_NS)
def test_plain_fp32_emulation_passes_every_case(n):
    worst = dict(p=0.0, m=0.0, v=0.0)
    for case in U.opt_cases(n):
        state, sc, dm = U.case_state(case)
        r = U.adamw_ratios(U.plain_adamw(case), state, sc, dm)
        for k in worst:
            worst[k] = max(worst[k], r[k])
            assert r[k] <= 1.0, (case, k, r[k])
    print(f'plain AdamW n={n}: worst ratios {worst}')


def test_plain_fp32_emulation_passes_the_large_case():
    state, sc, dm = U.case_state(U.OPT_BIG)
    r = U.adamw_ratios(U.plain_adamw(U.OPT_BIG), state, sc, dm)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize('mut', U.MUTATIONS)
def test_every_mutation_is_rejected_at_its_planted_case(mut):
    case, key = U.mutation_table()[mut]
    state, sc, dm = U.case_state(case)
    assert abs(dm - 0.95) < 1e-7
    good = U.adamw_ratios(U.plain_adamw(case), state, sc, dm)
    assert all(v <= 1.0 for v in good.values()), good
    bad = U.adamw_ratios(U.plain_adamw(case, mut), state, sc, dm)
    assert bad[key] > 1.0, (mut, bad)
    if key == 'p':          # m and v do not see the decay: a mutation of it alone leaves them exact
        assert bad['m'] <= 1.0 and bad['v'] <= 1.0, bad


def test_the_reference_without_a_decay_is_adam_ref_and_dm_is_rounded_once():
    case = U.OptCase(1023, 2, 1e-3, None, 0.5, 0.999, True)
    state, sc, dm = U.case_state(case)
    assert dm is None
    (p1, _, _), (tp, _, _) = U.adamw_ref(state, sc, None)
    (q1, _, _), (tq, _, _) = U.adam_ref(state, sc)
    assert torch.equal(p1, q1) and torch.equal(tp, tq)
    assert U.decay_mul(1e-3, 1e-2) == float(torch.tensor(1.0 - 1e-3 * 1e-2, dtype=torch.float64).float())
    assert U.decay_mul(1e-9, 1e-9) == 1.0          # below half an ulp of 1: the multiplier is exactly 1


# ---------------------------------------------------------------------------------------------- 2. C ABI
def test_new_symbols_declared_exported_and_bound():
    from patchgan_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'patchgan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(pg_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the clip forms' arguments plus the decay multiplier (a launch argument; the _dev form reads it from the scalars)
    assert len(_lib.SIGNATURES['pg_adamw_step'][1]) == len(_lib.SIGNATURES['pg_adam_clip_step'][1]) + 1
    assert _lib.SIGNATURES['pg_adamw_step_dev'][1] == _lib.SIGNATURES['pg_adam_clip_step_dev'][1]


def test_argument_validation_before_any_launch():
    from patchgan_amd import _lib
    lib = _lib.load()
    a = 1 << 20           # a non-NULL, 16-byte-aligned address that is never dereferenced: every call below is refused on the host

    def arg(p=a, g=a, m=a, v=a, ema=None, n=4099, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, bc1=0.1, sbc2=0.03, dm=0.99, ed=0.0, stat=None):
        return lib.pg_adamw_step(p, g, m, v, ema, n, lr, b1, b2, eps, bc1, sbc2, dm, ed, stat, None)

    def dev(p=a, g=a, m=a, v=a, ema=None, n=4099, b1=0.9, b2=0.999, eps=1e-8, sc=a, ed=0.0, stat=None):
        return lib.pg_adamw_step_dev(p, g, m, v, ema, n, b1, b2, eps, sc, ed, stat, None)
    for f in (arg, dev):
        for k in ('p', 'g', 'm', 'v'):
            assert f(**{k: None}) == -1, k
            assert f(**{k: a + 4}) == -1, k
        assert f(ema=a + 8, ed=0.5) == -1 and f(stat=a + 4) == -1
        for n in (0, -4):
            assert f(n=n) == -1
        for bad in (NAN, -0.1, 1.0, 1.5, INF):
            assert f(b1=bad) == -1 and f(b2=bad) == -1, bad
        for bad in (NAN, -0.1, 1.0, INF):
            assert f(ema=a, ed=bad) == -1, bad
            assert f(ema=a, ed=bad, stat=a) == -1, bad
    for bad in (NAN, 0.0, -0.5, 1.0000001, 2.0, INF, -INF):
        assert arg(dm=bad) == -1, bad
        assert arg(dm=bad, ema=a, ed=0.5, stat=a) == -1, bad
    for bad in (0.0, -1.0, NAN):
        assert arg(bc1=bad) == -1 and arg(sbc2=bad) == -1
    assert dev(sc=None) == -1


# ---------------------------------------------------------------------------------------------- 3. settings
def test_check_betas_and_weight_decay():
    from patchgan_amd import engine as E
    assert E.check_betas(None) == ((0.9, 0.999), (0.9, 0.999))
    assert E.check_betas((0.5, 0.999)) == ((0.5, 0.999), (0.5, 0.999))
    assert E.check_betas([[0.5, 0.999], (0, 0.9)]) == ((0.5, 0.999), (0.0, 0.9))
    for bad in (0.5, 'a', (0.5,), (0.5, 0.9, 0.9), (1.0, 0.9), (0.5, 1.0), (-0.1, 0.9), (NAN, 0.9), (0.5, INF), (True, 0.9), ('0.5', 0.9),
                ((0.5, 0.9), None), ((0.5, 0.9), (0.5, 1.0)), (0.5, 1.0 - 1e-12), ((0.5, 0.9), 0.9)):
        with pytest.raises(ValueError):
            E.check_betas(bad)
    assert E.check_weight_decay(None) == (None, None)
    assert E.check_weight_decay(0) == (None, None) and E.check_weight_decay(0.0) == (None, None)
    assert E.check_weight_decay(1e-2) == (1e-2, 1e-2)
    assert E.check_weight_decay((1e-2, None)) == (1e-2, None) and E.check_weight_decay([None, 0.5]) == (None, 0.5)
    assert E.check_weight_decay((0, 0.5)) == (None, 0.5)
    for bad in (-1e-3, NAN, INF, 'a', True, (1e-2,), (1e-2, 1e-2, 1e-2), (1e-2, -1.0), (NAN, None)):
        with pytest.raises(ValueError):
            E.check_weight_decay(bad)
    assert E.decay_mul(0.1, 0.5) == 1.0 - 0.1 * 0.5
    for lr, wd in ((0.1, 10.0), (1.0, 1.0), (0.5, 4.0)):
        with pytest.raises(ValueError):
            E.decay_mul(lr, wd)
    # the third scalar of a captured step
    sc = E.adam_scalars(3, 0.1, 0.5, 0.999, 0.5)
    assert len(sc) == 3 and float(sc[2]) == U.decay_mul(0.1, 0.5) and sc[:2] == E.adam_scalars(3, 0.1, 0.5, 0.999)
    assert tuple(float(x) for x in sc[:2]) == U.scalars(3, 0.1, 0.5, 0.999)[3:]


def test_yaml_forms():
    from patchgan_amd import train as T
    tp = yaml.safe_load("betas: [0.5, 0.999]\nweight_decay: 0.01\nsave_optimizer: true\ngen_learning_rate: 0.001\ndisc_learning_rate: 0.002\n")
    assert T._optimizer_of_params(tp) == ((0.5, 0.999), 0.01, True)
    tp = yaml.safe_load("betas: {gen: [0.5, 0.999], disc: [0.0, 0.9]}\nweight_decay: [0.01, null]\n")
    assert T._optimizer_of_params(tp) == (((0.5, 0.999), (0.0, 0.9)), (0.01, None), None)
    assert T._optimizer_of_params(yaml.safe_load("betas: {disc: [0.0, 0.9]}\n"))[0] == ((0.9, 0.999), (0.0, 0.9))
    assert T._optimizer_of_params({}) == (None, None, None)
    for text in ("betas: [0.5]", "betas: [0.5, 1.0]", "betas: {generator: [0.5, 0.9]}", "betas: {}", "betas: 0.5", "betas: {gen: [0.5, 2]}",
                 "weight_decay: -1", "weight_decay: [0.1]", "weight_decay: abc", "weight_decay: .nan", "save_optimizer: 3",
                 "weight_decay: 2000\ngen_learning_rate: 0.001", "weight_decay: [null, 100]\ndisc_learning_rate: 0.01"):
        with pytest.raises(ValueError):
            T._optimizer_of_params(yaml.safe_load(text))


def test_apply_train_params_and_trainer_checks(tmp_path):
    from patchgan_amd import train as T
    t = _trainer(tmp_path)
    assert t.betas is None and t.weight_decay is None and t.save_optimizer is None
    T.apply_train_params(t, dict(loss_type='tversky', seg_alpha=200, betas={'gen': [0.5, 0.999], 'disc': [0.0, 0.9]}, weight_decay=[0.01, None],
                                 save_optimizer=True))
    assert t.betas == ((0.5, 0.999), (0.0, 0.9)) and t.weight_decay == (0.01, None) and t.save_optimizer is True
    assert t._optim_now() == (((0.5, 0.999), (0.0, 0.9)), (0.01, None))
    T.apply_train_params(t, dict(loss_type='tversky', seg_alpha=200))
    assert t.betas is None and t.weight_decay is None and t.save_optimizer is None
    assert t._optim_now() == (((0.9, 0.999), (0.9, 0.999)), (None, None)) and t._optim_key() == ()
    # setup_optimizers() and batch() refuse bad settings before anything changes or runs
    x = torch.zeros(1, 3, 256, 256)
    for attr, bad in (('betas', (0.5, 1.0)), ('weight_decay', -1.0), ('weight_decay', 5000.0)):
        setattr(t, attr, bad)
        with pytest.raises(ValueError):
            t.setup_optimizers(1e-3, 1e-3)
        assert t._adam is None
        with pytest.raises(ValueError):
            t.batch(x, x[:, :1], train=True)
        setattr(t, attr, None)
    t.weight_decay = 5.0          # fine at 1e-3, refused at the learning rate setup_optimizers() is asked for
    with pytest.raises(ValueError):
        t.setup_optimizers(0.5, 1e-3)
    t.setup_optimizers(1e-3, 1e-3)
    assert t._adam is not None


def test_dispatch_and_kind_key(tmp_path, monkeypatch):
    """Which entry point _adam_step reaches (adam_spy: recorded at engine.adam_update), with which betas: a default trainer makes the
    calls of before with (0.9, 0.999); a network with a decay takes adamw_step with ema / stat as the other settings say."""
    from patchgan_amd import engine as E
    calls = S.spy(monkeypatch)
    t = _trainer(tmp_path)
    t.setup_optimizers(1e-3, 2e-3)
    t.generator.ensure_grad_flat(), t.discriminator.ensure_grad_flat()
    t._adam_step('g'), t._adam_step('d')
    assert [c[0] for c in calls] == ['adam_step', 'adam_step']
    assert S.step_lr(calls[0]) == (1, 1e-3) and S.step_lr(calls[1]) == (1, 2e-3)
    assert S.betas(calls[0]) == (0.9, 0.999) and S.betas(calls[1]) == (0.9, 0.999)      # the calls of before: torch.optim.Adam's betas
    assert all(c[2][k] is None for c in calls for k in ('scalars', 'ema', 'ema_decay', 'stat', 'weight_decay')) and calls[0][2]['eps'] == 1e-8
    del calls[:]
    t.betas = ((0.5, 0.999), (0.0, 0.9))
    t._adam_step('g'), t._adam_step('d')
    assert [c[0] for c in calls] == ['adam_step', 'adam_step']
    assert S.step_lr(calls[0]) == (2, 1e-3) and S.betas(calls[0]) == (0.5, 0.999)
    assert S.step_lr(calls[1]) == (2, 2e-3) and S.betas(calls[1]) == (0.0, 0.9)
    assert t._optim_key() == (('optim', ((0.5, 0.999), (0.0, 0.9)), (None, None)),)
    del calls[:]
    t.weight_decay = (1e-2, None)
    t._adam_step('g'), t._adam_step('d')
    assert [c[0] for c in calls] == ['adamw_step', 'adam_step']
    k = calls[0][2]
    assert S.step_lr(calls[0]) == (3, 1e-3) and (k['weight_decay'], k['ema'], k['ema_decay'], k['stat']) == (1e-2, None, None, None)
    assert S.betas(calls[0]) == (0.5, 0.999)
    del calls[:]
    t.gen_lr = 5e-4          # the multiplier follows the step's learning rate
    t.ema_decay, t.clip_grad_norm = 0.99, (1.0, None)
    t._ema_ensure(), monkeypatch.setattr(t, '_clip_ensure', lambda: True), monkeypatch.setattr(t, '_clip_stat', lambda w: 'STAT')
    t._clip = (None, None, None)
    t._adam_step('g')
    assert [c[0] for c in calls] == ['grad_norm', 'adamw_step']
    k = calls[1][2]
    assert S.step_lr(calls[1]) + (k['weight_decay'],) == (4, 5e-4, 1e-2) and k['ema'] is t._ema and (k['ema_decay'], k['stat']) == (0.99, 'STAT')
    assert S.betas(calls[1]) == (0.5, 0.999)
    del calls[:]
    # a step being captured: three floats per network, the network without a decay reads the first two of its three
    t._adam_dev = torch.arange(6.0)
    t._adam_step('g'), t._adam_step('d')
    assert [c[0] for c in calls] == ['grad_norm', 'adamw_step_dev', 'adam_step_dev']
    assert calls[1][2]['scalars'].tolist() == [0.0, 1.0, 2.0] and calls[2][2]['scalars'].tolist() == [3.0, 4.0, 5.0]
    t._t_g, t._t_d = 7, 9
    assert [float(x) for x in t._adam_scalars('g', 3)] == [float(x) for x in E.adam_scalars(7, 5e-4, 0.5, 0.999, 1e-2)]
    assert [float(x) for x in t._adam_scalars('d', 3)] == [float(x) for x in E.adam_scalars(9, 2e-3, 0.0, 0.9)] + [1.0]
    t._adam_dev = None


# ---------------------------------------------------------------------------------------------- 4. the optimizer file
def _fill(t, seed=11):
    gen = torch.Generator().manual_seed(seed)
    for buf in t._adam:
        buf.copy_(torch.rand(buf.numel(), generator=gen))
    t._t_g, t._t_d = 5, 4


@pytest.mark.parametrize('kind', ['plain', 'spectral', 'affine'])
def test_optimizer_file_loads_into_torch_and_back(tmp_path, kind):
    from patchgan_amd import engine as E
    t = _trainer(tmp_path, spectral=kind == 'spectral', affine=kind == 'affine')
    G, D = t.generator, t.discriminator
    t.betas, t.weight_decay, t.save_optimizer = ((0.5, 0.999), (0.0, 0.9)), (1e-2, None), True
    t.setup_optimizers(1e-3, 2e-3)
    _fill(t)
    sd = t.optimizer_state(7)
    assert set(sd) == {'format', 'gen', 'disc', 'trainer'} and sd['format'] == 1
    assert sd['trainer'] == dict(epoch=7, gen_lr=1e-3, dsc_lr=2e-3, t_g=5, t_d=4, step=0, diffaug_counter=None, plateau=None)
    opts = []
    for net, sec, cls, (m, v), steps, lr, betas, wd in ((G, sd['gen'], torch.optim.AdamW, t._adam[0:2], 5, 1e-3, (0.5, 0.999), 1e-2),
                                                        (D, sd['disc'], torch.optim.Adam, t._adam[2:4], 4, 2e-3, (0.0, 0.9), 0.0)):
        params = list(net.parameters())
        names = [k for k, _ in net.named_parameters()]
        if kind == 'spectral' and net is D:
            assert any(k.endswith('weight_orig') for k in names)
        if kind == 'affine':
            assert len(names) > len(net._layers) * (2 if net is D else 1)
        opt = cls(params)
        opt.load_state_dict(sec)          # as it is
        grp = opt.param_groups[0]
        assert (grp['lr'], tuple(grp['betas']), grp['eps'], grp['weight_decay'], grp['amsgrad']) == (lr, betas, 1e-8, wd, False)
        mv, vv = E.torch_views(m, net._layers), E.torch_views(v, net._layers)
        assert len(opt.state) == len(params) == len(sec['state'])
        for i, (k, p) in enumerate(zip(names, params)):
            st = opt.state[p]
            assert st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == steps
            assert sec['state'][i]['exp_avg'].is_contiguous() and sec['state'][i]['exp_avg'].shape == p.shape
            assert torch.equal(st['exp_avg'], mv[k]) and torch.equal(st['exp_avg_sq'], vv[k]), k
        opts.append(opt)
    # the reverse: a file whose sections come straight from torch optimizers
    path = str(tmp_path / 'from_torch.pth')
    torch.save({'gen': opts[0].state_dict(), 'disc': opts[1].state_dict()}, path)
    t2 = _trainer(tmp_path / 'b', spectral=kind == 'spectral', affine=kind == 'affine')
    t2.load_optimizer_state(path)
    assert t2._adam is None and t2._resume is not None
    t2.setup_optimizers(3e-4, 4e-4)          # consumes the pending state: moments and step counts kept, this call's learning rates
    assert t2._resume is None and (t2._t_g, t2._t_d) == (5, 4) and (t2.gen_lr, t2.dsc_lr) == (3e-4, 4e-4)
    for net, a, b in ((G, t._adam[0], t2._adam[0]), (G, t._adam[1], t2._adam[1]), (D, t._adam[2], t2._adam[2]), (D, t._adam[3], t2._adam[3])):
        va, vb = E.torch_views(a, net._layers), E.torch_views(b, net._layers)
        assert all(torch.equal(va[k], vb[k]) for k in va)
    t2.setup_optimizers(3e-4, 4e-4)          # nothing pending: fresh
    assert (t2._t_g, t2._t_d) == (0, 0) and not any(bool(b.any()) for b in t2._adam)


def test_optimizer_file_errors_and_trainer_section(tmp_path):
    t = _trainer(tmp_path)
    t.save_optimizer = True
    t.diffaug = 'translation,cutout'
    t.setup_optimizers(1e-3, 2e-3)
    _fill(t)
    t._step = 6
    t._aug_counter = torch.tensor([6], dtype=torch.int64)
    from patchgan_amd.trainer import _Plateau
    t._plateau = [_Plateau(1e-3), _Plateau(2e-3)]
    t._plateau[0].best, t._plateau[0].bad = 0.25, 3
    sd = t.optimizer_state(2)
    assert sd['trainer']['diffaug_counter'] == 6 and sd['trainer']['step'] == 6
    assert sd['trainer']['plateau'] == [dict(lr=1e-3, best=0.25, bad=3), dict(lr=2e-3, best=INF, bad=0)]
    t2 = _trainer(tmp_path / 'b')
    t2.load_optimizer_state(sd)
    t2.setup_optimizers(1e-3, 2e-3)
    assert t2._step == 6 and int(t2._aug_counter[0]) == 6 and t2._resume_plateau == sd['trainer']['plateau']
    from patchgan_amd import engine as E
    for net, a, b in zip((t.generator,) * 2 + (t.discriminator,) * 2, t._adam, t2._adam):          # (parameters only: the flat buffer's pad floats are no state)
        va, vb = E.torch_views(a, net._layers), E.torch_views(b, net._layers)
        assert all(torch.equal(va[k], vb[k]) for k in va)
    # wrong parameter count / shape
    bad = {'gen': sd['disc'], 'disc': sd['disc']}
    with pytest.raises(RuntimeError):
        t2.load_optimizer_state(bad)
    import copy
    bad = copy.deepcopy(sd)
    bad['gen']['state'][0]['exp_avg'] = torch.zeros(3)
    with pytest.raises(RuntimeError):
        t2.load_optimizer_state(bad)
    with pytest.raises(RuntimeError):
        t2.load_optimizer_state({'generator': 1})
    assert t2._resume is None


def test_save_and_load_last_checkpoint_files(tmp_path, capsys):
    """Off: save() writes the two files of before and load_last_checkpoint() ignores an optimizer file.  On: the third file, read back
    as a pending state; a missing file prints one line and resumes as before."""
    t = _trainer(tmp_path)
    t.setup_optimizers(1e-3, 2e-3)
    _fill(t)
    t.save(1)
    assert sorted(os.listdir(tmp_path)) == ['discriminator_ep_001.pth', 'generator_ep_001.pth']
    t.save_optimizer = True
    t.save(2)
    assert sorted(os.listdir(tmp_path)) == ['discriminator_ep_001.pth', 'discriminator_ep_002.pth', 'generator_ep_001.pth', 'generator_ep_002.pth',
                                            'optimizer_ep_002.pth']
    t2 = _trainer(tmp_path, seed=4)
    t2.load_last_checkpoint()          # off: the file is not read
    assert t2.start == 3 and t2._resume is None
    t2.save_optimizer = True
    t2.load_last_checkpoint()
    assert t2._resume is not None and t2._resume['t_g'] == 5 and 'optimizer_ep_002.pth' in capsys.readouterr().out
    os.remove(tmp_path / 'optimizer_ep_002.pth')
    t3 = _trainer(tmp_path, seed=4)
    t3.save_optimizer = True
    t3.load_last_checkpoint()
    out = capsys.readouterr().out
    assert t3.start == 3 and t3._resume is None and 'optimizers start fresh' in out and 'Checkpoints not loaded' not in out
