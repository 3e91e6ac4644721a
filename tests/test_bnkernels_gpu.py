"""Every BatchNorm kernel variant of batchnorm.hip on the MI355X, per element against float64 (references, tolerances, launch-plan
mirror and case table: tests/bn_util.py, held to float64 autograd and to the seeded mutations in tests/test_bnkernels_cpu.py).  The
C ABI is called directly on NaN-filled strided offset views: the fused forward / backward pair and its halves on every row in training
mode (one and two segments) and in evaluation mode, the split form as two emulated ranks, partial sums made on the host, the
running-statistics update, and the refusals.  Every test prints the worst ratio per (entry point, path, quantity); the coverage guard
asserts, when the whole file ran, that every path of every entry point was launched in vector and in scalar form."""

import pytest
import torch

from tests import bn_util as B
from tests import normact_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PG_OK, PG_EINVAL, PG_EWORKSPACE = 0, -1, -2
NAN = float('nan')

CASES = B.cases()
BY = {c.name: c for c in CASES}
SPLIT_ROWS = ('2x8x4x4', '2x8x4x4-mis', '2x64x24x24', '2x4x64x65-mis', '2x12x23x25', '2x12x23x25-mis')
PART_ROWS = (1, 15, 16, 17, 40)         # Ns * chunks around the 16 rows k_bn_merge sums per pass
ALL_TESTS = ({('fused', c.name) for c in CASES} | {('split', n) for n in SPLIT_ROWS} | {('parts', s) for s in (1, 2)}
             | {('running',), ('refusals',)})
_LAUNCHED = set()       # (entry point, path, VEC) and (entry point, 'unrolled-partial' / 'unrolled-apply') this session launched
_RAN = set()
_WORST = {}             # (entry point, path, quantity) -> worst ratio


def _lib():
    from patchgan_amd import _lib as L
    return L, L.load()


def _note(case, entry, res, N=None):
    """Record the launch (what bn_util.bn_path says the entry point did with the case's views) and its ratios."""
    pl = B.bn_path(case, entry, N)
    _LAUNCHED.add((entry, pl['path'], pl['vec']))
    for k in ('unrolled_partial', 'unrolled_apply'):
        if pl[k]:
            _LAUNCHED.add((entry, k.replace('_', '-')))
    for q, v in res.items():
        key = (entry, pl['path'], q)
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    return pl


class V:
    """An (N, HW, C) fp32 channel slice of a wider NaN-filled buffer: pixel stride ld > C, element offset off (normact_util.LAYOUT:
    'al' 16-byte aligned with ld % 4 == C % 4, 'mis' an odd offset and ld = C + 3)."""

    def __init__(self, N, HW, C, layout, x=None):
        pad, self.off = U.LAYOUT[layout][False]
        self.N, self.HW, self.C, self.ld = N, HW, C, C + pad
        self.buf = torch.full((N * HW * self.ld + self.off + 64,), NAN, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        if x is not None:
            self.inner().copy_(x.reshape(N * HW, C).float().to(DEV))

    def inner(self):
        return self.buf[self.off:self.off + self.N * self.HW * self.ld].view(self.N * self.HW, self.ld)[:, :self.C]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def read(self):
        return self.inner().double().cpu().reshape(self.N, self.HW, self.C)

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())

    def rest_nan(self):
        m = torch.ones_like(self.buf, dtype=torch.bool)
        m[self.off:self.off + self.N * self.HW * self.ld].view(self.N * self.HW, self.ld)[:, :self.C] = False
        return bool(torch.isnan(self.buf[m]).all())


def _flat(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=DEV)


def _params(*vs):
    """fp32 vectors in one NaN-filled device buffer at 4-byte (not 16-byte) aligned addresses, as the blocks of a flat buffer sit."""
    C = vs[0].numel()
    t = _flat(len(vs) * (C + 1) + 1)
    ptrs = []
    for i, v in enumerate(vs):
        o = 1 + i * (C + 1)
        t[o:o + C] = v.float().to(DEV)
        ptrs.append(t.data_ptr() + 4 * o)
    return t, ptrs


class Rig:
    """The device side of one (sub-)batch of a row: y, g1, g2 in the row's layout, the parameters, a workspace of the queried size."""

    def __init__(self, case, inp, rows=None):
        L, self.lib = _lib()
        self.case = case
        N, C, H, W = case.shape
        sel = (lambda t: t) if rows is None else (lambda t: t[rows])
        y, g1, g2 = sel(inp['y']), sel(inp['g1']), sel(inp['g2'])
        self.N, self.C, self.HW = y.shape[0], C, H * W
        self.vy, self.vg1, self.vg2 = (V(self.N, self.HW, C, case.layout, t) for t in (y, g1, g2))
        self.keep_params, (self.wp, self.bp, self.rmp, self.rvp) = _params(inp['w'], inp['b'], inp['rm'], inp['rv'])
        self.seed = B.seed_of(case)

    def ws(self, nseg):
        n = int(self.lib.pg_batchnorm_workspace_bytes(self.N, self.HW, self.C, nseg))
        assert n == B.workspace_bytes(self.N, self.HW, self.C, nseg) and n > 0
        t = torch.empty(n, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t

    def out_view(self):
        return V(self.N, self.HW, self.C, self.case.layout)

    def fwd(self, nseg, act, p, halves=False):
        """pg_batchnorm_act_fwd, or its halves pg_batchnorm_stats + pg_batchnorm_act_apply."""
        N, C, HW, lib, vy = self.N, self.C, self.HW, self.lib, self.vy
        vo, coef, bstat, ws = self.out_view(), _flat(nseg * C * 4), _flat(nseg * C * 2, torch.float64), self.ws(nseg)
        code = U.ACT_CODE[act]
        if halves:
            assert lib.pg_batchnorm_stats(vy.ptr(), vy.ld, None, 0, self.wp, self.bp, coef.data_ptr(), bstat.data_ptr(), N, HW, C, nseg, 1e-5,
                                          ws.data_ptr(), ws.numel(), None) == PG_OK
            assert lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo.ptr(), vo.ld, coef.data_ptr(), N, HW, C, nseg, code, p, self.seed, None) == PG_OK
        else:
            assert lib.pg_batchnorm_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, self.wp, self.bp, coef.data_ptr(), bstat.data_ptr(), N, HW, C, nseg,
                                            code, 1e-5, p, self.seed, ws.data_ptr(), ws.numel(), None) == PG_OK
        torch.cuda.synchronize()
        assert vo.rest_nan()
        return dict(coef=coef.cpu().view(nseg, C, 4), bstat=bstat.cpu().view(nseg, C, 2), out=vo.read(), coef_dev=coef)

    def eval_fwd(self, act, p):
        """pg_batchnorm_eval_coef + pg_batchnorm_act_apply with one segment."""
        N, C, HW, lib, vy = self.N, self.C, self.HW, self.lib, self.vy
        vo, coef = self.out_view(), _flat(C * 4)
        assert lib.pg_batchnorm_eval_coef(self.rmp, self.rvp, self.wp, self.bp, C, 1e-5, coef.data_ptr(), None) == PG_OK
        assert lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo.ptr(), vo.ld, coef.data_ptr(), N, HW, C, 1, U.ACT_CODE[act], p, self.seed, None) == PG_OK
        torch.cuda.synchronize()
        assert vo.rest_nan()
        return dict(coef=coef.cpu().view(1, C, 4), out=vo.read(), coef_dev=coef)

    def g2_args(self, g2on):
        return (self.vg2.ptr(), self.vg2.ld) if g2on else (None, 0)

    def bwd(self, coef_dev, nseg, train, act, p, g2on, grads=True):
        N, C, HW, lib, vy, vg1 = self.N, self.C, self.HW, self.lib, self.vy, self.vg1
        vd, dg, ws = self.out_view(), _flat(2 * C + 2), self.ws(nseg)
        dwp, dbp = (dg.data_ptr() + 4, dg.data_ptr() + 4 * (C + 2)) if grads else (None, None)
        g2p, g2ld = self.g2_args(g2on)
        before = coef_dev.clone()
        assert lib.pg_batchnorm_act_bwd(vg1.ptr(), vg1.ld, g2p, g2ld, vy.ptr(), vy.ld, coef_dev.data_ptr(), vd.ptr(), vd.ld, dwp, dbp, N, HW, C,
                                        nseg, 1 if train else 0, U.ACT_CODE[act], p, self.seed, ws.data_ptr(), ws.numel(), None) == PG_OK
        torch.cuda.synchronize()
        assert vd.rest_nan() and torch.equal(coef_dev, before)
        if not grads:
            assert bool(torch.isnan(dg).all())
            return dict(dy=vd.read())
        assert bool(torch.isnan(dg[0])) and bool(torch.isnan(dg[C + 1]))
        return dict(dy=vd.read(), dweight=dg[1:C + 1].double().cpu(), dbias=dg[C + 2:].double().cpu())


def _show(tag, results):
    worst = {}
    for r in results.values():
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f'ratio bn {tag}', ' '.join(f'{k} {v:.4f}' for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ the fused pair, its halves, evaluation
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_fused_pair_and_evaluation_mode(case):
    """Every mode of the row (training with its segment counts: pg_batchnorm_act_fwd / _bwd; evaluation: pg_batchnorm_eval_coef,
    pg_batchnorm_act_apply, pg_batchnorm_act_bwd with train = 0) and every (activation, p, g2) of it: coef, bstat, out, dy, dweight,
    dbias within bn_util's per-element tolerances -- the chunked path with its K term, the one-workgroup path without.  Where the
    forward is chunked, pg_batchnorm_stats + pg_batchnorm_act_apply give its bits; on one-workgroup rows the halves (always the
    partial-sum kernels) are held to the chunked bounds.  With dweight == dbias == NULL dy keeps its bits."""
    inp = B.inputs(case)
    assert inp['left'] == 0
    rig = Rig(case, inp)
    for train, nseg in B.modes(case):
        results = {}
        chunked = B.bn_path(case, 'act_fwd')['path'] != 'one-wg'
        for i, (act, p, g2on) in enumerate(B.combos(case)):
            ref, plain = B.evaluate(case, inp, train, nseg, act, p, g2on)
            if train:
                f = rig.fwd(nseg, act, p)
                r = B.ratios(ref, plain, f, chunked)
                _note(case, 'act_fwd', r)
                if i == 0 or case.large:
                    h = rig.fwd(nseg, act, p, halves=True)
                    if chunked:
                        for k in ('coef', 'bstat', 'out'):
                            assert torch.equal(h[k], f[k]), (k, act, p, int((h[k] != f[k]).sum()))
                    rh = B.ratios(ref, plain, h, True)
                    _note(case, 'stats', {k: v for k, v in rh.items() if k != 'out'})
                    _note(case, 'act_apply', {'out': rh['out']})
                    r.update({'halves-' + k: v for k, v in rh.items()})
            else:
                f = rig.eval_fwd(act, p)
                r = B.ratios(ref, plain, f, False)
                _note(case, 'act_apply', {'out': r['out']})
                _LAUNCHED.add(('eval_coef', 'called', 0))
                for k in ('mean', 'rstd', 'scale', 'shift'):
                    _WORST['eval_coef', 'called', k] = max(_WORST.get(('eval_coef', 'called', k), 0.0), r[k])
            bw = rig.bwd(f['coef_dev'], nseg, train, act, p, g2on)
            rb = B.ratios(ref, plain, bw, chunked and train)
            _note(case, 'act_bwd', rb)
            r.update(rb)
            if i == len(B.combos(case)) - 1:
                none = rig.bwd(f['coef_dev'], nseg, train, act, p, g2on, grads=False)
                assert torch.equal(none['dy'], bw['dy'])
            results[act, p, g2on] = r
        _show(f"{case.name} {'train' if train else 'eval'} nseg={nseg}", results)
        bad = {k: v for k, v in results.items() if not max(v.values()) <= 1.0}
        assert not bad, (train, nseg, bad)
    _RAN.add(('fused', case.name))


# ------------------------------------------------------------------------------------------------ the split form, two emulated ranks
@pytest.mark.parametrize('name', SPLIT_ROWS)
def test_split_form_as_two_ranks(name):
    """pg_batchnorm_moments_fwd -> (host sum of the two ranks' moments) -> pg_batchnorm_coef_from_moments -> pg_batchnorm_act_apply,
    pg_batchnorm_moments_bwd -> (host sum) -> pg_batchnorm_bwd_apply, one sample per rank, against the float64 reference of the WHOLE
    batch with the same per-element tolerances (K granted: the coefficients come from E[x^2] - mean^2 on every path); every rank draws
    the dropout mask of ITS element indices.  The local forward moments within n * 2^-53 * sum |term|; the summed backward moments as
    dbias / dweight; the ranks' local dweight / dbias sum to the whole batch's."""
    case = BY[name]
    N, C, H, W = case.shape
    HW, world = H * W, 2
    Nl = N // world
    inp = B.inputs(case)
    lib = _lib()[1]
    rigs = [Rig(case, inp, slice(r * Nl, (r + 1) * Nl)) for r in range(world)]
    count = float(N * HW)
    results = {}
    for act, p, g2on in B.combos(case):
        code, seed = U.ACT_CODE[act], B.seed_of(case)
        keep = torch.cat([U.mask_t(seed, (Nl, HW, C), p)] * world)
        ref, plain = B.evaluate(case, inp, True, 1, act, p, g2on, keep=keep)
        moms, r = [], {}
        for k, rig in enumerate(rigs):
            mom, ws = _flat(C * 2, torch.float64), rig.ws(1)
            assert lib.pg_batchnorm_moments_fwd(rig.vy.ptr(), rig.vy.ld, None, 0, mom.data_ptr(), Nl, HW, C, 1, ws.data_ptr(), ws.numel(), None) == PG_OK
            torch.cuda.synchronize()
            yl = inp['y'][k * Nl:(k + 1) * Nl]
            loc = B.bn_ref(yl, None, None, inp['w'], inp['b'], act, 0.0, seed)
            rl = {'moments': U.worst_ratio(mom.cpu().view(1, C, 2), loc['moments'], B.tol_moments(loc, Nl * HW))}
            _note(case, 'moments_fwd', rl, N=Nl)
            r['moments'] = max(r.get('moments', 0.0), rl['moments'])
            moms.append(mom)
        mom = moms[0] + moms[1]
        coef, bstat = _flat(C * 4), _flat(C * 2, torch.float64)
        assert lib.pg_batchnorm_coef_from_moments(mom.data_ptr(), count, rigs[0].wp, rigs[0].bp, 1e-5, coef.data_ptr(), bstat.data_ptr(), C, 1,
                                                  None) == PG_OK
        _LAUNCHED.add(('coef_from_moments', 'called', 0))
        outs = []
        for rig in rigs:
            vo = rig.out_view()
            assert lib.pg_batchnorm_act_apply(rig.vy.ptr(), rig.vy.ld, vo.ptr(), vo.ld, coef.data_ptr(), Nl, HW, C, 1, code, p, seed, None) == PG_OK
            torch.cuda.synchronize()
            assert vo.rest_nan()
            outs.append(vo.read())
        rf = B.ratios(ref, plain, dict(coef=coef.cpu().view(1, C, 4), bstat=bstat.cpu().view(1, C, 2), out=torch.cat(outs)), True)
        _note(case, 'act_apply', {'out': rf['out']}, N=Nl)
        for k in ('mean', 'rstd', 'scale', 'shift', 'bmean', 'bvar'):
            _WORST['coef_from_moments', 'called', k] = max(_WORST.get(('coef_from_moments', 'called', k), 0.0), rf[k])
        r.update(rf)
        bmoms, dws, dbs = [], [], []
        for rig in rigs:
            bm, dg, ws = _flat(C * 2, torch.float64), _flat(2 * C), rig.ws(1)
            g2p, g2ld = rig.g2_args(g2on)
            assert lib.pg_batchnorm_moments_bwd(rig.vg1.ptr(), rig.vg1.ld, g2p, g2ld, rig.vy.ptr(), rig.vy.ld, coef.data_ptr(), bm.data_ptr(),
                                                dg.data_ptr(), dg.data_ptr() + 4 * C, Nl, HW, C, 1, code, p, seed, ws.data_ptr(), ws.numel(),
                                                None) == PG_OK
            torch.cuda.synchronize()
            assert torch.equal(dg[:C], bm.view(C, 2)[:, 1].float()) and torch.equal(dg[C:], bm.view(C, 2)[:, 0].float())
            bmoms.append(bm), dws.append(dg[:C].double().cpu()), dbs.append(dg[C:].double().cpu())
        bmom = bmoms[0] + bmoms[1]
        bm = bmom.cpu().view(1, C, 2)
        rm = {'s1': U.worst_ratio(bm[..., 0].reshape(1, 1, C), ref['s1'], B.tol_s1(ref, plain['s1'], True)),
              's2': U.worst_ratio(bm[..., 1].reshape(1, 1, C), ref['s2'], B.tol_s2(ref, plain['s2'], True)),
              'dweight': U.worst_ratio(dws[0] + dws[1], ref['dweight'], B.tol_dweight(ref, plain['dweight'], True)),
              'dbias': U.worst_ratio(dbs[0] + dbs[1], ref['dbias'], B.tol_dbias(ref, plain['dbias'], True))}
        _note(case, 'moments_bwd', rm, N=Nl)
        r.update(rm)
        dys = []
        for rig in rigs:
            vd, ws = rig.out_view(), rig.ws(1)
            g2p, g2ld = rig.g2_args(g2on)
            assert lib.pg_batchnorm_bwd_apply(rig.vg1.ptr(), rig.vg1.ld, g2p, g2ld, rig.vy.ptr(), rig.vy.ld, coef.data_ptr(), bmom.data_ptr(),
                                              count, vd.ptr(), vd.ld, Nl, HW, C, 1, code, p, seed, ws.data_ptr(), ws.numel(), None) == PG_OK
            torch.cuda.synchronize()
            assert vd.rest_nan()
            dys.append(vd.read())
        rd = B.ratios(ref, plain, dict(dy=torch.cat(dys)), True)
        _note(case, 'bwd_apply', rd, N=Nl)
        r.update(rd)
        results[act, p, g2on] = r
    _show(f'{name} split', results)
    bad = {k: v for k, v in results.items() if not max(v.values()) <= 1.0}
    assert not bad, bad
    _RAN.add(('split', name))


# ------------------------------------------------------------------------------------------------ partial sums from the host
@pytest.mark.parametrize('nseg', (1, 2))
def test_partial_sums_from_the_host(nseg):
    """pg_batchnorm_stats and pg_batchnorm_moments_fwd with `part` made on the host from random chunk bounds (y == NULL, no
    workspace): Ns * chunks below, at and above the 16 rows a lane group of the merge kernels sums per pass, 20 channels (a second,
    ragged merge workgroup)."""
    lib = _lib()[1]
    HW, C = 63, 20
    worst = {}
    for Ns, rows in [(1, r) for r in PART_ROWS] + [(2, 16), (2, 40)]:
        chunks, N = rows // Ns, nseg * Ns
        gen = torch.Generator().manual_seed(100 + rows + Ns)
        y = (0.5 + 2.0 * torch.randn((N, HW, C), generator=gen, dtype=torch.float32)).double()
        w, b = B.bn_params(C)
        ref = B.bn_ref(y, None, None, w, b, 'none', 0.0, 0, nseg)
        part = U.host_partials(y, U.chunk_bounds(HW, chunks)).to(DEV)
        assert part.shape == (N, chunks, C, 2) and part.is_contiguous()
        keep, (wp, bp) = _params(w, b)
        coef, bstat, mom = _flat(nseg * C * 4), _flat(nseg * C * 2, torch.float64), _flat(nseg * C * 2, torch.float64)
        assert lib.pg_batchnorm_stats(None, C, part.data_ptr(), chunks, wp, bp, coef.data_ptr(), bstat.data_ptr(), N, HW, C, nseg, 1e-5, None, 0,
                                      None) == PG_OK
        assert lib.pg_batchnorm_moments_fwd(None, C, part.data_ptr(), chunks, mom.data_ptr(), N, HW, C, nseg, None, 0, None) == PG_OK
        torch.cuda.synchronize()
        r = B.ratios(ref, None, dict(coef=coef.cpu().view(nseg, C, 4), bstat=bstat.cpu().view(nseg, C, 2)), True)
        r['moments'] = U.worst_ratio(mom.cpu().view(nseg, C, 2), ref['moments'], B.tol_moments(ref, Ns * HW))
        print(f'ratio bn host partials nseg={nseg} Ns={Ns} chunks={chunks}', ' '.join(f'{k} {v:.4f}' for k, v in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            ep = 'moments_fwd' if k == 'moments' else 'stats'
            _WORST[ep, 'host-part', k] = max(_WORST.get((ep, 'host-part', k), 0.0), v)
        _LAUNCHED.update({('stats', 'host-part', 0), ('moments_fwd', 'host-part', 0)})
    assert max(worst.values()) <= 1.0, worst
    _RAN.add(('parts', nseg))


# ------------------------------------------------------------------------------------------------ running statistics
def test_update_running():
    """pg_batchnorm_update_running with 1 and 3 layers (6, 300 and 64 channels), 1 and 2 slots: the header's recurrence in float64 on
    the device's own bstat, eps32 |value| per element; the counter is added to; the buffers' surroundings stay NaN."""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(9)
    worst = 0.0
    for Cs in ((6,), (6, 300, 64)):
        for nslots in (1, 2):
            items = (L.BnUpdateItem * len(Cs))()
            held = []
            for it, C in zip(items, Cs):
                bstat = torch.stack([torch.randn((nslots, C), generator=gen, dtype=torch.float64) * 3,
                                     torch.rand((nslots, C), generator=gen, dtype=torch.float64) * 4 + 0.1], -1).contiguous()
                rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
                run = _flat(2 * C + 3)
                run[1:1 + C], run[2 + C:2 + 2 * C] = rm0.to(DEV), rv0.to(DEV)
                cnt = torch.tensor([-1, 5, -1], dtype=torch.int64, device=DEV)
                bs = bstat.to(DEV)
                it.bstat, it.C = bs.data_ptr(), C
                it.running_mean, it.running_var = run.data_ptr() + 4, run.data_ptr() + 4 * (2 + C)
                it.num_batches_tracked = cnt.data_ptr() + 8
                held.append((bstat, rm0, rv0, run, cnt, bs, C))
            assert lib.pg_batchnorm_update_running(len(Cs), items, nslots, 0.1, None) == PG_OK
            torch.cuda.synchronize()
            for bstat, rm0, rv0, run, cnt, bs, C in held:
                want_m, want_v = B.running_ref(bs.cpu(), rm0, rv0)
                r = B.running_ratio(run[1:1 + C].double().cpu(), run[2 + C:2 + 2 * C].double().cpu(), want_m, want_v)
                worst = max(worst, r)
                assert cnt.tolist() == [-1, 5 + nslots, -1]
                assert bool(torch.isnan(run[0])) and bool(torch.isnan(run[1 + C])) and bool(torch.isnan(run[2 + 2 * C]))
                assert torch.equal(bs.cpu(), bstat)
    print('ratio bn update_running', f'{worst:.4f}')
    _LAUNCHED.add(('update_running', 'called', 0))
    _WORST['update_running', 'called', 'running'] = worst
    assert worst <= 1.0
    assert lib.pg_batchnorm_update_running(0, items, 1, 0.1, None) == PG_EINVAL
    assert lib.pg_batchnorm_update_running(L.BN_MAX_LAYERS + 1, items, 1, 0.1, None) == PG_EINVAL
    assert lib.pg_batchnorm_update_running(1, items, 0, 0.1, None) == PG_EINVAL
    _RAN.add(('running',))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    """The header's codes, nothing written: a workspace one byte short (PG_EWORKSPACE, whatever kernel the views would select), nseg =
    3, N % nseg != 0, a count (or a segment) of one value, one of dweight / dbias NULL (PG_EINVAL)."""
    lib = _lib()[1]
    case = BY['2x8x4x4']
    inp = B.inputs(case)
    rig = Rig(case, inp)
    N, C, HW, vy, vg1, vg2 = rig.N, rig.C, rig.HW, rig.vy, rig.vg1, rig.vg2
    coef_ok = rig.fwd(1, 'leaky', 0.0)['coef_dev']
    mom_ok = torch.ones(2 * C * 2, dtype=torch.float64, device=DEV)

    def calls(N, nseg, ws_cut=0, count=None, dwn=False, dbn=False, cfm=True):
        """Every entry point that takes this geometry, with fresh NaN outputs: [(name, code, outputs)]."""
        vo, vd = V(max(N, 1), HW, C, case.layout), V(max(N, 1), HW, C, case.layout)
        ns = min(max(nseg, 1), 2)
        coef, bstat, mom, dg = _flat(ns * C * 4), _flat(ns * C * 2, torch.float64), _flat(ns * C * 2, torch.float64), _flat(2 * C)
        ws = rig.ws(1 if nseg == 3 or N % max(nseg, 1) else nseg)
        wsb = ws.numel() - ws_cut
        dwp, dbp = (None if dwn else dg.data_ptr()), (None if dbn else dg.data_ptr() + 4 * C)
        cnt = float(N * HW) if count is None else count
        out = []
        if count is None and not (dwn or dbn):
            out += [('act_fwd', lib.pg_batchnorm_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, rig.wp, rig.bp, coef.data_ptr(), bstat.data_ptr(), N, HW, C,
                                                         nseg, 1, 1e-5, 0.0, 7, ws.data_ptr(), wsb, None)),
                    ('stats', lib.pg_batchnorm_stats(vy.ptr(), vy.ld, None, 0, rig.wp, rig.bp, coef.data_ptr(), bstat.data_ptr(), N, HW, C, nseg, 1e-5,
                                                     ws.data_ptr(), wsb, None)),
                    ('moments_fwd', lib.pg_batchnorm_moments_fwd(vy.ptr(), vy.ld, None, 0, mom.data_ptr(), N, HW, C, nseg, ws.data_ptr(), wsb, None))]
            if not ws_cut:
                out.append(('act_apply', lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo.ptr(), vo.ld, coef_ok.data_ptr(), N, HW, C, nseg, 1, 0.0, 7, None)))
        if count is None:
            out += [('act_bwd', lib.pg_batchnorm_act_bwd(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, coef_ok.data_ptr(), vd.ptr(), vd.ld,
                                                         dwp, dbp, N, HW, C, nseg, 1, 1, 0.0, 7, ws.data_ptr(), wsb, None)),
                    ('moments_bwd', lib.pg_batchnorm_moments_bwd(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, coef_ok.data_ptr(),
                                                                 mom.data_ptr(), dwp, dbp, N, HW, C, nseg, 1, 0.0, 7, ws.data_ptr(), wsb, None))]
        if not (dwn or dbn):
            out.append(('bwd_apply', lib.pg_batchnorm_bwd_apply(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, coef_ok.data_ptr(),
                                                                mom_ok.data_ptr(), cnt, vd.ptr(), vd.ld, N, HW, C, nseg, 1, 0.0, 7, ws.data_ptr(),
                                                                wsb, None)))
            if cfm and not ws_cut:                               # (pg_batchnorm_coef_from_moments takes no N)
                out.append(('coef_from_moments', lib.pg_batchnorm_coef_from_moments(mom_ok.data_ptr(), cnt, rig.wp, rig.bp, 1e-5, coef.data_ptr(),
                                                                                    bstat.data_ptr(), C, nseg, None)))
        torch.cuda.synchronize()
        clean = vo.all_nan() and vd.all_nan() and all(bool(torch.isnan(t).all()) for t in (coef, bstat, mom, dg))
        return out, clean

    for what, kw, code, n in (('workspace one byte short', dict(N=N, nseg=1, ws_cut=1), PG_EWORKSPACE, 6),
                              ('nseg = 3', dict(N=N, nseg=3), PG_EINVAL, 8),
                              ('N % nseg != 0', dict(N=1, nseg=2, cfm=False), PG_EINVAL, 7),
                              ('count <= 1', dict(N=N, nseg=1, count=1.0), PG_EINVAL, 2),
                              ('dweight NULL, dbias given', dict(N=N, nseg=1, dwn=True), PG_EINVAL, 2),
                              ('dbias NULL, dweight given', dict(N=N, nseg=1, dbn=True), PG_EINVAL, 2)):
        got, clean = calls(**kw)
        print(what, got)
        assert len(got) == n and all(rc == code for _, rc in got), (what, got)
        assert clean, what
    # one value per (segment, channel): 2 x 512 x 1 x 1 as two segments is refused where batch statistics are formed
    c1 = BY['2x512x1x1']
    r1 = Rig(c1, B.inputs(c1))
    vo, coef, bstat, ws = r1.out_view(), _flat(2 * 512 * 4), _flat(2 * 512 * 2, torch.float64), r1.ws(2)
    assert lib.pg_batchnorm_act_fwd(r1.vy.ptr(), r1.vy.ld, vo.ptr(), vo.ld, r1.wp, r1.bp, coef.data_ptr(), bstat.data_ptr(), 2, 1, 512, 2, 1, 1e-5,
                                    0.0, 7, ws.data_ptr(), ws.numel(), None) == PG_EINVAL
    assert lib.pg_batchnorm_stats(r1.vy.ptr(), r1.vy.ld, None, 0, r1.wp, r1.bp, coef.data_ptr(), bstat.data_ptr(), 2, 1, 512, 2, 1e-5, ws.data_ptr(),
                                  ws.numel(), None) == PG_EINVAL
    torch.cuda.synchronize()
    assert vo.all_nan() and bool(torch.isnan(coef).all()) and bool(torch.isnan(bstat).all())
    _LAUNCHED.add(('workspace_bytes', 'called', 0))
    _RAN.add(('refusals',))


# ------------------------------------------------------------------------------------------------ coverage guard
def planned():
    """What the whole file must have launched: every path of every entry point that has it, in vector and scalar form, the unrolled
    loops of k_bn_partial and of the fixed k_bn_apply forward and backward, the host-partial routes and the entry points without a
    path -- eleven entry points, all that include/patchgan_hip.h declares for BatchNorm."""
    want = set()
    for e in ('act_fwd', 'act_bwd', 'moments_fwd', 'moments_bwd'):
        want |= {(e, p, v) for p in ('one-wg', 'chunked-fixed', 'chunked-flat') for v in (4, 1)}
    for e in ('stats', 'act_apply', 'bwd_apply'):
        want |= {(e, p, v) for p in ('chunked-fixed', 'chunked-flat') for v in (4, 1)}
    want |= {('act_fwd', 'unrolled-partial'), ('act_fwd', 'unrolled-apply'), ('act_bwd', 'unrolled-partial'), ('act_bwd', 'unrolled-apply'),
             ('stats', 'unrolled-partial'), ('act_apply', 'unrolled-apply'), ('bwd_apply', 'unrolled-apply')}
    want |= {('stats', 'host-part', 0), ('moments_fwd', 'host-part', 0)}
    want |= {(e, 'called', 0) for e in ('eval_coef', 'coef_from_moments', 'update_running', 'workspace_bytes')}
    return want


def test_coverage_guard():
    """The plan of the case table (bn_util.bn_path, tied to the library's workspace query on the CPU) contains every planned launch;
    when the whole file ran, every one of them was launched.  Prints the worst ratio per (entry point, path, quantity)."""
    want = planned()
    table = set()
    for c in CASES:
        for e in ('act_fwd', 'act_bwd', 'stats', 'act_apply'):
            pl = B.bn_path(c, e)
            table.add((e, pl['path'], pl['vec']))
            table |= {(e, k.replace('_', '-')) for k in ('unrolled_partial', 'unrolled_apply') if pl[k]}
    for n in SPLIT_ROWS:
        for e in ('moments_fwd', 'moments_bwd', 'bwd_apply', 'act_apply'):
            pl = B.bn_path(BY[n], e, N=1)
            table.add((e, pl['path'], pl['vec']))
            table |= {(e, k.replace('_', '-')) for k in ('unrolled_partial', 'unrolled_apply') if pl[k]}
    missing = {w for w in want if len(w) == 2 or w[1] not in ('called', 'host-part')} - table
    assert not missing, sorted(missing)
    print(f'{"entry point":20s} {"path":16s} {"quantity":12s} worst ratio')
    for (e, p, q), v in sorted(_WORST.items()):
        print(f'{e:20s} {p:16s} {q:12s} {v:.4f}')
    if _RAN >= ALL_TESTS:
        assert want <= _LAUNCHED, sorted(want - _LAUNCHED)
        assert max(_WORST.values()) <= 1.0
    else:
        print('partial run: launch coverage not asserted;', len(ALL_TESTS - _RAN), 'tests did not run')
