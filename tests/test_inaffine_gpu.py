"""Affine InstanceNorm (functools.partial(nn.InstanceNorm2d, affine=True)) on the MI355X: the pg_instnorm_affine_act_* kernels per
element against float64 (references, tolerances and cases: tests/inaffine_util.py, held to torch autograd and to the seeded mutations
in tests/test_inaffine_cpu.py), the networks against the reference's fixtures (tests/golden/make_golden_ina.py), the launch modes,
bf16, data parallelism, what surrounds the step, and both CLIs.  Every test prints the figures it asserts."""
import functools
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests import inaffine_util as A
from tests import normact_util as U
from tests.golden_util import GOLDEN_DIR, LOSS_KEYS, probe, probe_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PG_OK = 0
AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)


def _lib():
    from patchgan_amd import _lib as L
    return L.load()


# ------------------------------------------------------------------------------------------------ kernels
def _geom(x):
    return (x.shape[0], 1, x.shape[1], x.shape[2])


def _gin(x, layout, bf):
    """(guarded view, guard) holding x ((N, HW, C) float64 values representable in the storage type)."""
    from tests import guard_util as G
    N, H, W, C = _geom(x)
    pad, off = U.LAYOUT[layout][bf]
    return G.view_from(x.reshape(N, H, W, C).permute(0, 3, 1, 2), ld=C + pad, off=off, bf=bf)


def _gout(like, layout, bf):
    from tests import guard_util as G
    N, H, W, C = _geom(like)
    pad, off = U.LAYOUT[layout][bf]
    return G.view(N, H, W, C, ld=C + pad, off=off, bf=bf)


def _read(v, like):
    from tests import guard_util as G
    return G.read_nchw(v).permute(0, 2, 3, 1).reshape(like.shape).cpu()


def _params(gamma, beta):
    """gamma, beta in one device buffer at 4-byte (not 16-byte) aligned addresses, as the blocks of a flat buffer may sit."""
    C = gamma.numel()
    t = torch.full((2 * C + 2,), float('nan'), device=DEV)
    t[1:1 + C] = gamma.float().to(DEV)
    t[2 + C:2 + 2 * C] = beta.float().to(DEV)
    gp, bp = t.data_ptr() + 4, t.data_ptr() + 4 * (2 + C)
    assert gp % 16 != 0 and gp % 4 == 0
    return t, gp, bp


class _Setup:
    def __init__(self, case, y, g1, g2):
        self.lib, self.case = _lib(), case
        N, C, H, W = case.shape
        self.N, self.C, self.HW = N, C, H * W
        by, bo, bg, bd = U.MIX[case.mix]
        self.vy, self.vg1, self.vg2 = _gin(y, case.layout, by)[0], _gin(g1, case.layout, bg)[0], _gin(g2, case.layout, bg)[0]
        full = int(self.lib.pg_instnorm_affine_workspace_bytes(N, self.HW, C))
        assert full == A.workspace_bytes(N, self.HW, C)
        self.ws = torch.empty(full, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 16 == 0
        self.plain_ws = int(self.lib.pg_instnorm_workspace_bytes(N, self.HW, C))
        self.like = y

    def affine(self, gp, bp, act, p, g2on, seed, grads=True, dgrad=None):
        """Forward then backward: dict of out, stats, dy, dgamma, dbeta on the host.  dgrad: a NaN-filled [2 C] tensor to use."""
        lib, case, N, C, HW = self.lib, self.case, self.N, self.C, self.HW
        by, bo, bg, bd = U.MIX[case.mix]
        code = U.ACT_CODE[act]
        vo, vd = _gout(self.like, case.layout, bo)[0], _gout(self.like, case.layout, bd)[0]
        stats = torch.full((N * C * 2,), float('nan'), device=DEV)
        rc = lib.pg_instnorm_affine_act_fwd_t(self.vy.ptr(), self.vy.ld, vo.ptr(), vo.ld, gp, bp, stats.data_ptr(), N, HW, C, code, 1e-5, p,
                                              seed, self.ws.data_ptr(), self.ws.numel(), None, (1 if by else 0) | (2 if bo else 0))
        assert rc == PG_OK
        torch.cuda.synchronize()
        st = stats.cpu().view(N, C, 2)
        dg = torch.full((2 * C,), float('nan'), device=DEV) if dgrad is None else dgrad
        g2p, g2ld = (self.vg2.ptr(), self.vg2.ld) if g2on else (None, 0)
        rc = lib.pg_instnorm_affine_act_bwd_t(self.vg1.ptr(), self.vg1.ld, g2p, g2ld, self.vy.ptr(), self.vy.ld, gp, bp, stats.data_ptr(),
                                              vd.ptr(), vd.ld, dg.data_ptr() if grads else None, dg.data_ptr() + 4 * C if grads else None,
                                              N, HW, C, code, p, seed, self.ws.data_ptr(), self.ws.numel(), None,
                                              (3 if bg else 0) | (4 if by else 0) | (8 if bd else 0))
        assert rc == PG_OK
        torch.cuda.synchronize()
        assert torch.equal(stats.cpu().view(N, C, 2), st)
        return dict(out=_read(vo, self.like), stats=st, dy=_read(vd, self.like), dgamma=dg[:C].cpu() if grads else None,
                    dbeta=dg[C:].cpu() if grads else None, raw=dg)

    def plain(self, act, p, g2on, seed):
        lib, case, N, C, HW = self.lib, self.case, self.N, self.C, self.HW
        by, bo, bg, bd = U.MIX[case.mix]
        code = U.ACT_CODE[act]
        vo, vd = _gout(self.like, case.layout, bo)[0], _gout(self.like, case.layout, bd)[0]
        stats = torch.full((N * C * 2,), float('nan'), device=DEV)
        wp, wb = self.ws.data_ptr(), self.plain_ws
        assert lib.pg_instnorm_act_fwd_t(self.vy.ptr(), self.vy.ld, vo.ptr(), vo.ld, stats.data_ptr(), N, HW, C, code, 1e-5, p, seed, wp, wb,
                                         None, (1 if by else 0) | (2 if bo else 0)) == PG_OK
        g2p, g2ld = (self.vg2.ptr(), self.vg2.ld) if g2on else (None, 0)
        assert lib.pg_instnorm_act_bwd_t(self.vg1.ptr(), self.vg1.ld, g2p, g2ld, self.vy.ptr(), self.vy.ld, stats.data_ptr(), vd.ptr(), vd.ld,
                                         N, HW, C, code, p, seed, wp, wb, None, (3 if bg else 0) | (4 if by else 0) | (8 if bd else 0)) == PG_OK
        torch.cuda.synchronize()
        return dict(out=_read(vo, self.like), stats=stats.cpu().view(N, C, 2), dy=_read(vd, self.like))


CASES = A.cases()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_affine_kernels_against_float64(case):
    """Every (activation, p, g2) of the case: out, stats, dy, d(gamma), d(beta) within inaffine_util's per-element tolerances; with
    dgamma == NULL a NaN-filled gradient buffer stays NaN and dy keeps its bits; a second run gives the same bits; with gamma = 1,
    beta = 0 out and dy are the plain entry points' bit for bit (zero tolerance)."""
    y, g1, g2, gamma, beta, left = A.inputs(case)
    assert left == 0
    s = _Setup(case, y, g1, g2)
    keep, gp, bp = _params(gamma, beta)
    keep1, gp1, bp1 = _params(torch.ones_like(gamma), torch.zeros_like(beta))
    seed = U.seed_of(case)
    results = {}
    for act, p, g2on in U.combos(case):
        h2 = g2 if g2on else None
        got = s.affine(gp, bp, act, p, g2on, seed)
        ref = A.affine_ref(y, g1, h2, gamma, beta, act, p, seed)
        plain = A.plain_affine(y, g1, h2, gamma, beta, act, p, seed)
        results[act, p, g2on] = A.ratios(case, ref, plain, got)
        again = s.affine(gp, bp, act, p, g2on, seed)
        assert torch.equal(again['raw'], got['raw']) and torch.equal(again['dy'], got['dy']) and torch.equal(again['out'], got['out'])
        none = s.affine(gp, bp, act, p, g2on, seed, grads=False)
        assert bool(torch.isnan(none['raw']).all()) and torch.equal(none['dy'], got['dy'])
        ident, twin = s.affine(gp1, bp1, act, p, g2on, seed), s.plain(act, p, g2on, seed)
        for k in ('out', 'stats', 'dy'):
            assert torch.equal(ident[k], twin[k]), (k, act, p, g2on, int((ident[k] != twin[k]).sum()))
    worst = {k: max(r[k] for r in results.values()) for k in ('fwd', 'mean', 'rstd', 'dy', 'dgamma', 'dbeta')}
    for k, v in worst.items():
        print(f'ratio affine {k} {case.name} {v:.4f}')
    bad = {k: v for k, v in results.items() if not max(v.values()) <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize('geom', [(4, 32, 32, 128, 64, 2), (2, 64, 64, 64, 32, 2)], ids=lambda g: 'x'.join(map(str, g)))
def test_statistics_from_a_conv_epilogue(geom):
    """The conv epilogue's partial sums (pg_instnorm_affine_act_fwd_parts_t) against the stand-alone route over the conv's output, as
    tests/test_batchnorm_gpu.py demands of BatchNorm: outputs and statistics within 1e-6 of their largest value."""
    from patchgan_amd import engine as E, _lib as L
    from tests.gpu_util import to_view, empty_view, pack
    N, Hb, Wb, Ca, Cb, s = geom
    g = torch.Generator().manual_seed(3)
    big = torch.randn(N, Cb, Hb, Wb, generator=g)
    Wt = torch.randn(Ca, Cb, 4, 4, generator=g) / (Cb * 16) ** 0.5
    op = E.ConvOp(*geom, L.ALGO_AUTO | L.TUNE_WINO2_ALL)
    vin = to_view(big, ld=Cb + 4)
    y = empty_view(N, op.Hs, op.Ws, Ca, ld=Ca + 4, off=4)
    chunks = op.stats_chunks(0, vin, y)
    assert chunks > 0
    part = torch.empty(N * chunks * Ca * 2, dtype=torch.float64, device=DEV)
    op.big2small(vin, pack(Wt), 0, None, 0, y, part=part)
    gamma, beta = A.affine_params(Ca)
    flat = torch.cat([gamma.float(), beta.float()]).to(DEV)
    outs, stats = [], []
    for use_part in (True, False):
        out = empty_view(N, op.Hs, op.Ws, Ca, ld=Ca + 8, off=4)
        st = torch.full((N * Ca * 2,), float('nan'), device=DEV)
        E.instnorm_affine_act_fwd(y, out, st, flat, 0, Ca, 1, part=part if use_part else None, chunks=chunks)
        outs.append(out.to_nchw().double().cpu())
        stats.append(st.double().cpu())
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print('parts vs stand-alone: out', rel(outs[0], outs[1]), 'stats', rel(stats[0], stats[1]))
    assert rel(outs[0], outs[1]) < 1e-6 and rel(stats[0], stats[1]) < 1e-6
    z = (y.to_nchw().double().cpu() - stats[1].view(N, Ca, 2)[..., 0].view(N, Ca, 1, 1)) * stats[1].view(N, Ca, 2)[..., 1].view(N, Ca, 1, 1)
    want = nn.functional.leaky_relu(z * gamma.view(1, Ca, 1, 1) + beta.view(1, Ca, 1, 1), 0.2)
    assert rel(outs[0], want) < 1e-5


@pytest.mark.parametrize('name', ['2x12x24x24', '2x64x24x24-bf16', '2x12x15x15'])
def test_containment(name):
    """Each new entry point writes only out / dy / stats / its workspace / d(gamma) / d(beta): guarded buffers (tests/guard_util.py),
    ld > C and a channel offset, one fp32 and one bf16 case on the chunked path and the single-workgroup path."""
    from tests import guard_util as G
    case = [c for c in CASES if c.name == name][0]
    N, C, H, W = case.shape
    HW = H * W
    by, bo, bg, bd = U.MIX[case.mix]
    y, g1, g2, gamma, beta, _ = A.inputs(case)
    lib = _lib()
    ins = G.Inputs()
    (vy, gy), (vg1, gg1), (vg2, gg2) = _gin(y, case.layout, by), _gin(g1, case.layout, bg), _gin(g2, case.layout, bg)
    assert vy.ld > C and vy.off > 0
    ggam, gbet = G.flat_from(gamma.float()), G.flat_from(beta.float())
    for g_, nm in ((gy, 'y'), (gg1, 'g1'), (gg2, 'g2'), (ggam, 'gamma'), (gbet, 'beta')):
        ins.add(g_, nm)
    wsb = int(lib.pg_instnorm_affine_workspace_bytes(N, HW, C))
    dtf, dtb = (1 if by else 0) | (2 if bo else 0), (3 if bg else 0) | (4 if by else 0) | (8 if bd else 0)
    for p in (0.0, 0.2):
        (vo, go), (vd, gd) = _gout(y, case.layout, bo), _gout(y, case.layout, bd)
        gst, gws, gdg, gdb = G.flat(N * C * 8), G.flat(wsb), G.flat(C * 4), G.flat(C * 4)
        assert lib.pg_instnorm_affine_act_fwd_t(vy.ptr(), vy.ld, vo.ptr(), vo.ld, ggam.ptr(), gbet.ptr(), gst.ptr(), N, HW, C, 1, 1e-5, p, 7,
                                                gws.ptr(), wsb, None, dtf) == PG_OK
        assert lib.pg_instnorm_affine_act_bwd_t(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, ggam.ptr(), gbet.ptr(), gst.ptr(),
                                                vd.ptr(), vd.ld, gdg.ptr(), gdb.ptr(), N, HW, C, 1, p, 7, gws.ptr(), wsb, None, dtb) == PG_OK
        torch.cuda.synchronize()
        for g_, wr, nm in ((go, 'slice', 'out'), (gd, 'slice', 'dy'), (gst, 'all', 'stats'), (gws, 'all', 'ws'), (gdg, 'all', 'dgamma'),
                           (gdb, 'all', 'dbeta')):
            G.assert_untouched(g_, wr, f'affine {name} p={p} {nm}')
        assert bool(torch.isfinite(G.read_nchw(vo)).all()) and bool(torch.isfinite(G.read_nchw(vd)).all())
        assert bool(torch.isfinite(gdg.inner(torch.float32)).all()) and bool(torch.isfinite(gdb.inner(torch.float32)).all())
        # the parts route: partial sums of y over 3 arbitrary chunks
        bounds = U.chunk_bounds(HW, 3)
        gpart = G.flat_from(U.host_partials(y, bounds))
        snap = gpart.snapshot()
        (vo2, go2), gst2 = _gout(y, case.layout, bo), G.flat(N * C * 8)
        assert lib.pg_instnorm_affine_act_fwd_parts_t(vy.ptr(), vy.ld, vo2.ptr(), vo2.ld, ggam.ptr(), gbet.ptr(), gst2.ptr(), gpart.ptr(), 3,
                                                      N, HW, C, 1, 1e-5, p, 7, None, dtf) == PG_OK
        torch.cuda.synchronize()
        G.assert_untouched(go2, 'slice', f'affine parts {name} out')
        G.assert_untouched(gst2, 'all', f'affine parts {name} stats')
        G.assert_unchanged(gpart, snap, 'part')
        ins.check(f'affine {name} p={p}')


# ------------------------------------------------------------------------------------------------ networks against the fixtures
class INAGolden:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
        conv = lambda v: v == 'True' if v in ('True', 'False') else (int(v) if v.lstrip('-').isdigit() else v)
        self.cfg = {k: conv(v) for k, v in zip(self.z['cfg_keys'], self.z['cfg_vals'])}
        self.model_seed, self.nsteps = int(self.z['meta'][0]), int(self.z['meta'][1])

    def inputs(self):
        c = self.cfg
        g = torch.Generator().manual_seed(7)
        x = torch.rand(c['B'], c['in_nc'], c['size'], c['size'], generator=g)
        y = (torch.rand(c['B'], c['out_nc'], c['size'], c['size'], generator=g) > 0.7).float()
        return x, y

    def modules(self, norm_layer=AFFINE, load_affine=True):
        """The networks under the fixture's seed with the fixture's overwritten gamma / beta (load_affine; else the initial 1 / 0)."""
        import patchgan_amd as pg
        c = self.cfg
        torch.manual_seed(self.model_seed)
        g = pg.UNet(c['in_nc'], c['out_nc'], c['nf'], norm_layer=norm_layer, use_dropout=False, activation=c['activation'],
                    final_act=c['final_act'])
        d = pg.Discriminator(c['in_nc'] + c['out_nc'], c['ndf'], n_layers=c['n_layers'], norm=c['norm'], norm_layer=norm_layer)
        if load_affine and norm_layer is AFFINE:
            with torch.no_grad():
                for prefix, net in (('g0/', g), ('d0/', d)):
                    for l in net.engine.layers:
                        if l.norm_params:
                            for sfx in ('.weight', '.bias'):
                                net.state_dict()[l.norm_key + sfx].copy_(torch.from_numpy(self.z[prefix + 'full/' + l.norm_key + sfx]))
        return g, d

    def get(self, prefix):
        p = prefix + '/'
        return {k[len(p):]: self.z[k] for k in self.z.files if k.startswith(p)}


def _trainer(g, d, folder, loss_type, mode=None):
    import patchgan_amd as pg
    t = pg.Trainer(g, d, str(folder))
    t.loss_type = loss_type
    t.setup_optimizers(1e-3, 1e-3)
    if mode is not None:
        t.graph, t.two_streams, t.AUTO_FORCE = 'auto', 'auto', mode
    return t


def _rel_probe(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a[2:] - b[2:]).max() / max(np.abs(b[2:]).max(), 1e-30)


def _check_probes(gold, prefix, prefix64, tensors, floor, report):
    """Probes of `tensors` ({key: tensor}) against the fixture's, bounded as tests/test_batchnorm_gpu.py bounds them:
    max(floor, 4 x the reference's OWN largest fp32-vs-float64 distance over the same set of probes)."""
    p32, p64 = gold.get(prefix), gold.get(prefix64)
    env = max(_rel_probe(p32[k], p64[k]) for k in p32)
    for k in p32:
        report.append((prefix, k, _rel_probe(probe(tensors[k]), p64[k]) / max(floor, 4 * env)))


@pytest.mark.parametrize('name', ['ina_a', 'ina_b'])
def test_affine_networks_train_like_the_reference(name, tmp_path):
    """Forward probes, every parameter's gradient probe after step 1 (gamma / beta included), the 10-step curve within
    max(1e-4, 4 e_ref(step)) (e_ref: the reference's own fp32-vs-float64 distance, running maximum), the state probes after step 10 and
    the evaluation losses, every bound from the fixture."""
    gold = INAGolden(name)
    c = gold.cfg
    report = []
    g, d = gold.modules()
    g.to(DEV).train()
    d.to(DEV).train()
    x, y = gold.inputs()
    with torch.no_grad():
        gen0, hid0 = g(x.to(DEV), return_hidden=True)
        dfake = d(torch.cat((x.to(DEV), gen0), 1))
    for key, got in (('fwd/gen', gen0), ('fwd/hidden', hid0), ('fwd/disc_fake', dfake)):
        ok, e = probe_close(probe(got), gold.z[key], 1e-4)
        print(name, key, 'probe error', e)
        assert ok, (key, e)
    t = _trainer(g, d, tmp_path, c['loss_type'])
    losses = []
    for s in range(gold.nsteps):
        l = t.batch(x, y, train=True)
        losses.append([l[k] for k in LOSS_KEYS])
        if s == 0:
            t.flush()
            for pre, net in (('ggrad1', g), ('dgrad1', d)):
                grads = {k: p.grad for k, p in net.named_parameters()}
                assert set(gold.get(pre)) == set(grads) and (pre != 'ggrad1' or any('Norm' in k for k in grads))
                _check_probes(gold, pre, pre + '_64', grads, 2e-4, report)
    losses = np.array(losses)
    want, want64 = gold.z['losses'], gold.z['losses64']
    e_ref = np.maximum.accumulate(np.abs(want - want64).max(1))
    bound = np.maximum(1e-4, 4 * e_ref)
    err = np.abs(losses - want).max(1)
    print(name, 'loss error / max(1e-4, 4 e_ref(step)) per step', np.round(err / bound, 3), 'error', err, 'e_ref', e_ref)
    report.append(('losses', 'per step', float((err / bound).max())))
    t.flush()
    _check_probes(gold, 'gK', 'gK64', g.state_dict(), 2e-4, report)
    _check_probes(gold, 'dK', 'dK64', d.state_dict(), 2e-4, report)
    l = t.batch(x, y, train=False)
    got = np.array([l[k] for k in LOSS_KEYS])
    e_post = max(e_ref[-1], np.abs(gold.z['eval_losses'] - gold.z['eval_losses64']).max())
    report.append(('eval_losses', '', float(np.abs(got - gold.z['eval_losses']).max() / max(1e-4, 4 * e_post))))
    bad = [e for e in report if e[2] > 1.0]
    print(name, 'error / bound above 1:', bad, 'worst:', max(report, key=lambda e: e[2]))
    assert not bad, bad


def _run_mode(mode, steps=6):
    gold = INAGolden('ina_b')
    g, d = gold.modules()
    g.to(DEV)
    d.to(DEV)
    t = _trainer(g, d, tempfile.mkdtemp(), gold.cfg['loss_type'], mode)
    x, y = gold.inputs()
    losses = [dict(t.batch(x, y, train=True)) for _ in range(steps)]
    t.flush()
    state = {k: v.detach().clone().cpu() for k, v in list(g.state_dict().items()) + [('d.' + k, v) for k, v in d.state_dict().items()]}
    modes = t.decided_modes()
    t.release()
    return losses, state, modes


def test_step_is_bit_identical_across_launch_modes():
    """One stream, two streams and the captured graph (by decree; the mode takes over after the trainer's 3 warm steps, so 6 steps: 3
    of them in the mode): losses and weights of ina_b's network, bit for bit."""
    ref = _run_mode(None)
    for mode in ('eager1', 'eager2', 'graph'):
        got = _run_mode(mode)
        assert got[2] == [mode], got[2]
        assert got[0] == ref[0], mode
        for k in ref[1]:
            assert torch.equal(got[1][k], ref[1][k]), (mode, k)
    moved = [k for k in ref[1] if 'Norm' in k and k.endswith('bias') and ref[1][k].abs().sum() > 0]
    assert moved


def _curve(g, d, gold, steps):
    t = _trainer(g, d, tempfile.mkdtemp(), gold.cfg['loss_type'])
    x, y = gold.inputs()
    out = []
    for _ in range(steps):
        l = t.batch(x, y, train=True)
        out.append([l[k] for k in LOSS_KEYS])
    t.flush()
    t.release()
    return np.array(out)


def test_bf16_precision():
    """set_precision('bf16') on ina_a's network: 10 finite steps; with gamma = 1, beta = 0 the first bf16 forward is the plain bf16
    network's bit for bit; with the fixture's gamma / beta the distance of the bf16 curve to the fixture's float64 curve is held to
    2 x the distance of the PLAIN bf16 network to ITS float64 curve (also in the fixture): bf16 rounding (2^-9 per stored or multiplied
    value) dominates both, the affine transform adds two fp32 roundings per element and |gamma| <= 1.5 of amplification.
    Measured on an MI355X (EXPERIMENTS.md, "Affine InstanceNorm"): affine 1.88e-3, plain 7.70e-3, ratio 0.24."""
    gold = INAGolden('ina_a')
    x, _ = gold.inputs()
    g1, d1 = gold.modules(load_affine=False)
    gp, dp = gold.modules(norm_layer=nn.InstanceNorm2d)
    for net in (g1, d1, gp, dp):
        net.to(DEV).set_precision('bf16')
    with torch.no_grad():
        assert torch.equal(g1(x.to(DEV)), gp(x.to(DEV)))
    plain = _curve(gp, dp, gold, gold.nsteps)
    g, d = gold.modules()
    g.to(DEV).set_precision('bf16')
    d.to(DEV).set_precision('bf16')
    aff = _curve(g, d, gold, gold.nsteps)
    assert np.isfinite(aff).all() and np.isfinite(plain).all()
    d_aff = np.abs(aff - gold.z['losses64']).max()
    d_plain = np.abs(plain - gold.z['plain_losses64']).max()
    print('bf16 curve distance to float64: affine', d_aff, 'plain', d_plain, 'ratio', d_aff / d_plain)
    assert d_aff <= 2 * d_plain, (d_aff, d_plain)


def _dp_worker(rank, world, port, q, nsteps):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(4)
    from patchgan_amd.parallel import shard_batch
    gold = INAGolden('ina_b')
    g, d = gold.modules()
    g.cuda()
    d.cuda()
    t = _trainer(g, d, tempfile.mkdtemp(), gold.cfg['loss_type'])
    t.bucket_bytes = 64 << 10
    x, y = gold.inputs()
    xs, ys = shard_batch(x, y, rank, world)
    curve = []
    for s in range(nsteps):
        l = t.batch(xs, ys, train=True)
        curve.append([l[k] for k in LOSS_KEYS])
    t.flush()
    torch.cuda.synchronize()
    q.put((rank, np.array(curve), g.flat.cpu().numpy(), d.flat.cpu().numpy()))
    dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_process_curve():
    """Two gloo ranks on one GPU, one sample each (tests/test_dp_gpu.py's scheme): ina_b's curve within the single-process bound
    max(1e-4, 4 e_ref(step)); the weights of the two ranks equal bit for bit (gamma / beta gradients ride in the flat all-reduce)."""
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _collect
    gold = INAGolden('ina_b')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    nsteps = 5
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, nsteps)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, g0, d0), (_, c1, g1, d1) = res
    assert np.array_equal(g0, g1) and np.array_equal(d0, d1)
    want, want64 = gold.z['losses'][:nsteps], gold.z['losses64'][:nsteps]
    bound = np.maximum(1e-4, 4 * np.maximum.accumulate(np.abs(want - want64).max(1)))
    err = np.abs(c0 - want).max(1)
    print('dp2 affine: loss error / bound per step', np.round(err / bound, 3), err)
    assert (err <= bound).all() and np.allclose(c0, c1, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ around the step
def test_ema_and_clipping_see_gamma_and_beta(tmp_path):
    """ema_decay and clip_grad_norm = inf (coef == 1): the weights are the unclipped run's bit for bit, and gamma / beta of
    ema_generator have moved from 1 / 0 (and are not the trained ones)."""
    gold = INAGolden('ina_a')
    x, y = gold.inputs()
    runs = []
    for clip in (None, float('inf')):
        g, d = gold.modules(load_affine=False)
        g.to(DEV)
        d.to(DEV)
        import patchgan_amd as pg
        t = pg.Trainer(g, d, str(tmp_path))
        t.loss_type = gold.cfg['loss_type']
        t.ema_decay, t.clip_grad_norm = (0.5, clip) if clip is not None else (None, None)      # (the average starts with setup_optimizers)
        t.setup_optimizers(1e-3, 1e-3)
        for _ in range(3):
            t.batch(x, y, train=True)
        t.flush()
        runs.append((g.flat.clone(), d.flat.clone(), t))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    t = runs[1][2]
    ema, cur = t.ema_generator.state_dict(), t.generator.state_dict()
    assert list(ema) == list(cur)
    for k in ('encoder.1.model.DownNorm1.weight', 'decoder.2.model.UpNorm2.bias'):
        init = 1.0 if k.endswith('weight') else 0.0
        assert not torch.equal(ema[k], torch.full_like(ema[k], init)) and not torch.equal(ema[k], cur[k]), k


def test_predict_image_in_training_and_eval_mode():
    """Tiled inference with an affine generator is refused in no mode: a 320 x 288 image equals build_mask over plain forwards of
    its tiles, in training and in evaluation mode."""
    from patchgan_amd import engine as E
    from patchgan_amd.infer import predict_image
    from tests.gpu_util import to_view
    gold = INAGolden('ina_a')
    g, _ = gold.modules()
    g.to(DEV)
    image = torch.rand(3, 320, 288, generator=torch.Generator().manual_seed(2)).to(DEV)
    masks = []
    for train in (True, False):
        g.train(train)
        got = predict_image(g, image, 256, 0.5, 0.5)
        tiles = E.tiles_gather(image, 256, 0.5)
        with torch.no_grad():
            pred = g(tiles.to_nchw())
        want = E.tiles_blend(to_view(pred), (320, 288), 0.5, 0.5).cpu().numpy()
        assert tiles.N > 1 and np.array_equal(np.asarray(got), want)
        masks.append(want)
    assert np.array_equal(masks[0], masks[1])


def test_checkpoint_round_trip_on_the_device(tmp_path):
    gold = INAGolden('ina_b')
    x, y = gold.inputs()
    g, d = gold.modules()
    g.to(DEV)
    d.to(DEV)
    folder = str(tmp_path) + '/'
    t = _trainer(g, d, folder, gold.cfg['loss_type'])
    for _ in range(2):
        t.batch(x, y, train=True)
    t.save(2)
    sd = torch.load(folder + 'generator_ep_002.pth')
    assert list(sd) == list(gold.z['g0/keys']) and sd['encoder.0.model.DownNorm0.weight'].shape == (4,)
    g2, d2 = gold.modules(load_affine=False)
    g2.to(DEV)
    d2.to(DEV)
    t2 = _trainer(g2, d2, folder, gold.cfg['loss_type'])
    t2.load_last_checkpoint()
    assert torch.equal(g2.flat, g.flat) and torch.equal(d2.flat, d.flat)
    with torch.no_grad():
        assert torch.equal(g2(x.to(DEV)), g(x.to(DEV)))


# ------------------------------------------------------------------------------------------------ CLIs
@pytest.mark.parametrize('norm_layer', ['instance_affine', 'batch', None])
def test_train_then_infer_with_the_norm_layer_key(norm_layer, tmp_path, monkeypatch, capsys):
    """patchgan_train for one epoch on a generated 4-image dataset, then patchgan_infer with the same key, writes masks; with the key
    absent the printed summary and the checkpoint keys are the plain network's."""
    from patchgan_amd.train import patchgan_train
    from patchgan_amd.infer import patchgan_infer
    from tests.test_cli_gpu import PLUGIN
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'io.py').write_text(PLUGIN)
    gen = {'filters': 4, 'activation': 'leakyrelu', 'use_dropout': False}
    disc = {'filters': 4, 'n_layers': 3, 'norm': True}
    if norm_layer is not None:
        gen['norm_layer'] = disc['norm_layer'] = norm_layer
    cfg = {'dataset': {'type': 'Blobs', 'size': 256, 'in_channels': 3, 'out_channels': 1,
                       'train_data': {'images': '4', 'masks': ''}, 'validation_data': {'images': '2', 'masks': ''}},
           'model_params': {'generator': gen, 'discriminator': disc}, 'checkpoint_path': str(tmp_path / 'ckpt'),
           'train_params': {'loss_type': 'tversky', 'seg_alpha': 200, 'gen_learning_rate': 1e-3, 'disc_learning_rate': 1e-3,
                            'decay_rate': 0.9, 'save_freq': 1}}
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    G_ep, D_ep = patchgan_train(['-c', 'cfg.yaml', '-n', '1', '-b', '2', '--dataloader_workers', '0'])
    assert len(G_ep) == 1 and np.isfinite(G_ep).all() and np.isfinite(D_ep).all()
    out = capsys.readouterr().out
    sd = torch.load(tmp_path / 'ckpt' / 'generator_ep_001.pth')
    nkeys = {'instance_affine': 38, 'batch': 74, None: 14}[norm_layer]
    assert len(sd) == nkeys and f'parameters in {38 if norm_layer else 14} tensors' in out
    assert ('DownNorm0.weight' in out) == (norm_layer is not None)
    icfg = {'dataset': {'type': 'BlobsInfer', 'dataset_path': '2', 'size': 256},
            'model_params': {'generator': gen, 'discriminator': disc},
            'checkpoint_paths': {'generator': str(tmp_path / 'ckpt' / 'generator_ep_001.pth'),
                                 'discriminator': str(tmp_path / 'ckpt' / 'discriminator_ep_001.pth')},
            'infer_params': {'output_path': str(tmp_path / 'pred'), 'threshold': 0.5}}
    (tmp_path / 'icfg.yaml').write_text(yaml.safe_dump(icfg))
    patchgan_infer(['-c', 'icfg.yaml'])
    m = np.load(tmp_path / 'pred' / 'blob_001.npy')
    assert m.shape == (256, 256) and set(np.unique(m)) <= {0.0, 1.0}
