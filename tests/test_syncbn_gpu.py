"""nn.SyncBatchNorm on the MI355X: the split-form BatchNorm entry points (local moments -> sum across ranks -> coefficients / backward
apply) as two emulated ranks in one process against torch's batch_norm in float64 over the WHOLE batch; their containment; a
SyncBatchNorm pair without a process group bit-identical to a BatchNorm2d pair; and data-parallel training (two ranks over gloo on the
one GPU, a one-rank RCCL group) against the reference's BatchNorm fixtures -- a SyncBatchNorm layer under data parallelism IS
BatchNorm2d over the concatenated batch.  Bounds: those of tests/test_batchnorm_gpu.py for the same quantities."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import tests.test_batchnorm_gpu as B
from tests.golden_util import LOSS_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PG_OK, PG_EWORKSPACE = 0, -2


def _lib():
    from patchgan_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ws(lib, N, HW, C, nseg):
    return torch.empty(int(lib.pg_batchnorm_workspace_bytes(N, HW, C, nseg)), dtype=torch.uint8, device=DEV)


def _rank_rows(N, nseg, world):
    """Sample indices of each rank: global segment s is the union of every rank's segment s (rank r holds the r-th part of each)."""
    seg = N // nseg
    per = seg // world
    return [[s * seg + r * per + i for s in range(nseg) for i in range(per)] for r in range(world)]


# ------------------------------------------------------------------------------------------------ kernels, two emulated ranks
def _conv_halves(N, rows):
    """y = a stride-2 conv's output [N, 64, 64, 64] computed per rank on the polyphase Winograd path, with the epilogue's partial sums."""
    from patchgan_amd import engine as E, _lib as L
    from tests.gpu_util import to_view, empty_view, pack
    g = torch.Generator().manual_seed(3)
    big = torch.randn(N, 32, 128, 128, generator=g)
    Wt = torch.randn(64, 32, 4, 4, generator=g) / (32 * 16) ** 0.5
    P = pack(Wt)
    views, parts, x = [], [], torch.empty(N, 64, 64, 64)
    for r in rows:
        op = E.ConvOp(len(r), 128, 128, 64, 32, 2, L.ALGO_AUTO | L.TUNE_WINO2_ALL)
        vin = to_view(big[r], ld=36)
        y = empty_view(len(r), op.Hs, op.Ws, 64, ld=72, off=4)
        chunks = op.stats_chunks(0, vin, y)
        assert chunks > 0
        part = torch.empty(len(r) * chunks * 64 * 2, dtype=torch.float64, device=DEV)
        op.big2small(vin, P, 0, None, 0, y, part=part)
        views.append(y)
        parts.append((part, chunks))
        x[r] = y.to_nchw().cpu()
    return x, views, parts


# (shape, segments, activation, dropout, misaligned views, forward moments from a conv's partial sums)
SPLIT_CASES = [((2, 512, 1, 1), 1, 'relu', False, False, False),          # one value per channel and rank, two in the global batch
               ((4, 6, 5, 7), 1, 'leakyrelu', True, False, False),        # scalar path, odd sizes
               ((4, 6, 5, 7), 2, 'tanh', False, False, False),
               ((4, 32, 16, 16), 1, 'none', False, False, False),         # small planes: one launch per moments call
               ((4, 32, 16, 16), 2, 'leakyrelu', True, False, False),
               ((4, 32, 16, 16), 2, 'leakyrelu', True, True, False),      # views that are not 16-byte aligned
               ((4, 64, 64, 64), 1, 'leakyrelu', True, False, False),     # chunked vector path
               ((4, 64, 64, 64), 2, 'relu', False, False, False),
               ((4, 64, 64, 64), 1, 'leakyrelu', False, False, True)]


@pytest.mark.parametrize('case', SPLIT_CASES, ids=lambda c: f"{'x'.join(map(str, c[0]))}-s{c[1]}-{c[2]}{'-drop' if c[3] else ''}"
                                                           f"{'-misaligned' if c[4] else ''}{'-convpart' if c[5] else ''}")
def test_split_kernels_as_two_ranks_match_torch_float64_on_the_whole_batch(case):
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view, empty_view
    L, lib = _lib()
    (N, C, H, W), nseg, act, drop, mis, convpart = case
    HW, world = H * W, 2
    rows = _rank_rows(N, nseg, world)
    Nl = N // world
    g = torch.Generator().manual_seed(N * 7 + C + H)
    parts = None
    if convpart:
        x, vys, parts = _conv_halves(N, rows)
    else:
        x = torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3
        vys = [to_view(x[r], ld=C + 8, off=B._off(C, mis)) for r in rows]
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g) * 0.2
    rm0 = torch.randn(C, generator=g) * 0.1
    rv0 = torch.rand(C, generator=g) + 0.5
    l, flat, bufs, counters, scratch = B._layer(C)
    flat[l.g_off:l.g_off + C] = w.to(DEV)
    flat[l.be_off:l.be_off + C] = b.to(DEV)
    bufs[l.rm_off:l.rm_off + C] = rm0.to(DEV)
    bufs[l.rv_off:l.rv_off + C] = rv0.to(DEV)
    seed = 0x5EED1234 + C
    p = 0.2 if drop else 0.0
    count = float((N // nseg) * HW)                       # the GLOBAL number of values per (segment, channel)
    vos = [empty_view(Nl, H, W, C, ld=C + 12, off=B._off(C, mis)) for _ in rows]
    if mis:
        assert all(v.ptr() % 16 for v in vys + vos) and vys[0].ld % 4 == 0
    ws = _ws(lib, Nl, HW, C, nseg)

    # ---- forward: local moments per rank, their sum, coefficients with the global count, apply per rank
    moms = []
    for r, vy in enumerate(vys):
        mom = torch.full((nseg * C * 2,), float('nan'), dtype=torch.float64, device=DEV)
        if parts is not None:
            rc = lib.pg_batchnorm_moments_fwd(None, vy.ld, parts[r][0].data_ptr(), parts[r][1], mom.data_ptr(), Nl, HW, C, nseg, None, 0, _st())
        else:
            rc = lib.pg_batchnorm_moments_fwd(vy.ptr(), vy.ld, None, 0, mom.data_ptr(), Nl, HW, C, nseg, ws.data_ptr(), ws.numel(), _st())
        assert rc == PG_OK
        moms.append(mom)
    xl = [x[r].double().view(nseg, Nl // nseg, C, H, W) for r in rows]
    if parts is None:
        # the local moments themselves: fp64 sums of exactly representable terms in another order -- each within n * 2^-53 of sum |term|
        # (n <= 8192 here: 9.1e-13), and B._rel divides by the largest moment, sum x^2 >= sum |x| for these inputs
        for mom, xr in zip(moms, xl):
            want = torch.stack((xr.sum((1, 3, 4)), (xr * xr).sum((1, 3, 4))), -1).reshape(-1)
            assert B._rel(mom, want) <= 1e-12
    mom = moms[0] + moms[1]
    coef = torch.empty(nseg * C * 4, dtype=torch.float32, device=DEV)
    assert lib.pg_batchnorm_coef_from_moments(mom.data_ptr(), count, L.ptr(flat, l.g_off), L.ptr(flat, l.be_off), 1e-5, coef.data_ptr(),
                                              scratch.data_ptr(), C, nseg, _st()) == PG_OK
    for vy, vo in zip(vys, vos):
        assert lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo.ptr(), vo.ld, coef.data_ptr(), Nl, HW, C, nseg, B.ACTS[act], p, seed, _st()) == PG_OK

    # reference: torch's batch_norm in float64 per GLOBAL segment of the whole batch
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = torch.cat([F.batch_norm(xs, None, None, w64, b64, True, 0.1, 1e-5) for xs in x64.split(N // nseg)])
    a = B.TORCH_ACT[act](z)
    if drop:
        mask = torch.empty(N, C, H, W, dtype=torch.float64)
        half = B._mask(Nl, H, W, C, seed)                 # every rank draws the mask of ITS element indices under the seed it was given
        for r in rows:
            mask[r] = half
        a = a * mask / 0.8
    out = torch.empty(N, C, H, W, dtype=torch.float64)
    for r, vo in zip(rows, vos):
        out[r] = vo.to_nchw().double().cpu()
    assert B._rel(out, a.detach()) <= 1e-5

    # ---- backward, two gradient sources
    g1 = torch.randn(N, C, H, W, generator=g)
    g2 = torch.randn(N, C, H, W, generator=g)
    a.backward(g1.double() + g2.double())
    vg1 = [to_view(g1[r], ld=C + 8, off=B._off(C, mis, 2)) for r in rows]
    vg2 = [to_view(g2[r]) for r in rows]
    vdys = [empty_view(Nl, H, W, C, ld=C + 4, off=B._off(C, mis, 1)) for _ in rows]
    bmoms, dws, dbs = [], [], []
    for vy, a1, a2 in zip(vys, vg1, vg2):
        bm = torch.full((nseg * C * 2,), float('nan'), dtype=torch.float64, device=DEV)
        dw, db = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
        assert lib.pg_batchnorm_moments_bwd(a1.ptr(), a1.ld, a2.ptr(), a2.ld, vy.ptr(), vy.ld, coef.data_ptr(), bm.data_ptr(), dw.data_ptr(),
                                            db.data_ptr(), Nl, HW, C, nseg, B.ACTS[act], p, seed, ws.data_ptr(), ws.numel(), _st()) == PG_OK
        bmoms.append(bm), dws.append(dw), dbs.append(db)
    bmom = bmoms[0] + bmoms[1]
    for vy, a1, a2, vdy in zip(vys, vg1, vg2, vdys):
        assert lib.pg_batchnorm_bwd_apply(a1.ptr(), a1.ld, a2.ptr(), a2.ld, vy.ptr(), vy.ld, coef.data_ptr(), bmom.data_ptr(), count, vdy.ptr(),
                                          vdy.ld, Nl, HW, C, nseg, B.ACTS[act], p, seed, ws.data_ptr(), ws.numel(), _st()) == PG_OK
    dy = torch.empty(N, C, H, W, dtype=torch.float64)
    for r, vdy in zip(rows, vdys):
        dy[r] = vdy.to_nchw().double().cpu()
    assert B._rel(dy, x64.grad) <= 5e-5
    # the weight / bias gradients are LOCAL sums: their SUM over the ranks is the whole batch's gradient (a gradient all-reduce adds them)
    assert B._rel(dws[0].double() + dws[1].double(), w64.grad) <= 5e-5
    assert B._rel(dbs[0].double() + dbs[1].double(), b64.grad) <= 5e-5
    # ... and each equals the sums of its own moments over the segments
    for bm, dw, db in zip(bmoms, dws, dbs):
        m = bm.view(nseg, C, 2).sum(0)
        assert torch.equal(dw, m[:, 1].float()) and torch.equal(db, m[:, 0].float())

    # ---- the running statistics: the global mean, the variance unbiased with the GLOBAL count
    E.bn_update_running([l], bufs, counters, scratch, nseg)
    rm, rv = rm0.double(), rv0.double()
    for xs in x.double().split(N // nseg):
        rm = (0.9 * rm + 0.1 * xs.mean((0, 2, 3))).float().double()
        rv = (0.9 * rv + 0.1 * xs.var((0, 2, 3), unbiased=True)).float().double()
    assert B._rel(bufs[l.rm_off:l.rm_off + C], rm) <= 1e-6 and B._rel(bufs[l.rv_off:l.rv_off + C], rv) <= 1e-6
    assert int(counters[0]) == nseg


class _PeerDist:
    """A Dist for one emulated rank of `world`: the all-reduce adds the moments the test computed for the other rank."""
    on = True

    def __init__(self, world, peer=None):
        self.world, self.peer, self.calls = world, peer, 0

    def all_reduce_side(self, t, producers=()):
        self.calls += 1
        if self.peer is not None:
            t += self.peer
        return lambda: None


def test_the_more_than_one_value_check_uses_the_global_count():
    """(2, 512, 1, 1) as one sample per rank: each rank has ONE value per channel, the global batch two -- the engine's forward goes
    through; with one rank in the group (global count 1) it raises the reference's ValueError before any launch or collective."""
    from patchgan_amd import engine as E
    from tests.gpu_util import to_view, empty_view
    L, lib = _lib()
    C = 512
    g = torch.Generator().manual_seed(5)
    # the two values of a channel at least 1 apart: z = x * scale + shift in fp32 is off by about 2^-24 * |x| * rstd, and rstd = 2 / |x0 - x1|
    # for two values -- a channel whose values nearly coincide is ill-conditioned for ANY fp32 BatchNorm, not a case for a 1e-5 bound
    x0 = torch.randn(1, C, 1, 1, generator=g) * 1.5 + 0.3
    x = torch.cat((x0, x0 + (1 + torch.rand(1, C, 1, 1, generator=g)) * torch.sign(torch.randn(1, C, 1, 1, generator=g))))
    l, flat, bufs, counters, scratch = B._layer(C)
    flat[l.g_off:l.g_off + C] = 1.0
    vy, vo = to_view(x[:1], ld=C + 8, off=4), empty_view(1, 1, 1, C, ld=C + 12, off=4)
    peer_y = to_view(x[1:], ld=C + 8, off=4)
    peer = torch.empty(C * 2, dtype=torch.float64, device=DEV)
    ws = _ws(lib, 1, 1, C, 1)
    assert lib.pg_batchnorm_moments_fwd(peer_y.ptr(), peer_y.ld, None, 0, peer.data_ptr(), 1, 1, C, 1, ws.data_ptr(), ws.numel(), _st()) == PG_OK
    lone = _PeerDist(1)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        E.batchnorm_act_fwd(l, E.BNRun(True, bufs, scratch, 0, 1, lone), flat, vy, vo, B.ACTS['none'])
    assert lone.calls == 0
    pair = _PeerDist(2, peer)
    E.batchnorm_act_fwd(l, E.BNRun(True, bufs, scratch, 0, 1, pair), flat, vy, vo, B.ACTS['none'])
    assert pair.calls == 1
    want = F.batch_norm(x.double(), None, None, None, None, True, 0.1, 1e-5)
    assert B._rel(vo.to_nchw(), want[:1]) <= 1e-5
    # evaluation mode communicates nothing and uses the running statistics
    ev = _PeerDist(2, peer)
    bn = E.BNRun(False, bufs, scratch, 0, 1, ev)
    assert bn.dist is None
    E.batchnorm_act_fwd(l, bn, flat, vy, vo, B.ACTS['none'])
    assert ev.calls == 0


# ------------------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize('shape', [(4, 32, 16, 16), (2, 512, 1, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_split_entry_points_write_only_what_they_were_handed(shape):
    """The four split-form entry points with an exact workspace and guarded mom, coef, bstat, dweight, dbias and dy: only the declared
    bytes change, no input changes; a workspace one 256-byte step short returns PG_EWORKSPACE with nothing written.  Values (one
    rank: the local count is the global one) against float64 autograd at the per-kernel bounds."""
    from tests import guard_util as G
    L, lib = _lib()
    N, C, H, W = shape
    HW, nseg = H * W, 1
    gen = torch.Generator(device='cuda').manual_seed(2)
    y = (torch.randn(shape, device='cuda', generator=gen, dtype=torch.float64) * 2 + 0.5).float().double().requires_grad_(True)
    wt = (torch.rand(C, device='cuda', generator=gen, dtype=torch.float64) + 0.5).float().double().requires_grad_(True)
    bs = torch.randn(C, device='cuda', generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
    g1 = torch.randn(shape, device='cuda', generator=gen, dtype=torch.float64).float().double()
    want = F.leaky_relu(F.batch_norm(y, None, None, wt, bs, True, 0.1, 1e-5), 0.2)
    want.backward(g1)
    count = float(N * HW)
    full = int(lib.pg_batchnorm_workspace_bytes(N, HW, C, nseg))
    assert full >= 256
    ins = G.Inputs()
    vy, gy = G.view_from(y.detach(), ld=C + 4, off=0)
    ins.add(gy, 'y')
    w_g, b_g = ins.add(G.flat_from(wt.detach().float()), 'weight'), ins.add(G.flat_from(bs.detach().float()), 'bias')
    vg, gg = G.view_from(g1, ld=C + 4, off=4)
    ins.add(gg, 'g1')

    mom = None
    for claim in (full - 256, full):
        mom = G.flat(nseg * C * 2 * 8)
        ws = G.flat(full, back=max(full, G.BACK))
        rc = lib.pg_batchnorm_moments_fwd(vy.ptr(), vy.ld, None, 0, mom.ptr(), N, HW, C, nseg, ws.ptr(), claim, None)
        torch.cuda.synchronize()
        what = f'batchnorm_moments_fwd {shape} ws {claim}/{full}'
        if claim < full:
            assert rc == PG_EWORKSPACE, (what, rc)
            G.assert_untouched(mom, None, what), G.assert_untouched(ws, None, what)
        else:
            assert rc == PG_OK, (what, rc)
            G.assert_untouched(mom, 'all', what + ' mom'), G.assert_untouched(ws, claim, what + ' workspace')
        ins.check(what)
    ins.add(mom, 'mom')
    coef, bstat = G.flat(nseg * C * 4 * 4), G.flat(nseg * C * 2 * 8)
    what = f'batchnorm_coef_from_moments {shape}'
    assert lib.pg_batchnorm_coef_from_moments(mom.ptr(), 1.0, w_g.ptr(), b_g.ptr(), 1e-5, coef.ptr(), bstat.ptr(), C, nseg, None) == -1
    torch.cuda.synchronize()
    G.assert_untouched(coef, None, what + ' refused'), G.assert_untouched(bstat, None, what + ' refused')
    assert lib.pg_batchnorm_coef_from_moments(mom.ptr(), count, w_g.ptr(), b_g.ptr(), 1e-5, coef.ptr(), bstat.ptr(), C, nseg, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(coef, 'all', what + ' coef'), G.assert_untouched(bstat, 'all', what + ' bstat')
    ins.check(what)
    ins.add(coef, 'coef')
    yd = y.detach()
    st = bstat.inner(torch.float64).view(C, 2)
    assert B._rel(st[:, 0], yd.mean((0, 2, 3))) <= 1e-6 and B._rel(st[:, 1], yd.var((0, 2, 3), unbiased=True)) <= 1e-6
    vo, go = G.view(N, H, W, C, ld=C + 4, off=4)
    assert lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo.ptr(), vo.ld, coef.ptr(), N, HW, C, nseg, 1, 0.0, 0, None) == PG_OK
    torch.cuda.synchronize()
    assert B._rel(G.read_nchw(vo), want.detach()) <= 1e-5
    G.assert_untouched(go, 'slice', 'batchnorm_act_apply out')

    bmom = None
    for claim in (full - 256, full):
        bmom = G.flat(nseg * C * 2 * 8)
        dw, db = G.flat(C * 4), G.flat(C * 4)
        ws = G.flat(full, back=max(full, G.BACK))
        rc = lib.pg_batchnorm_moments_bwd(vg.ptr(), vg.ld, None, 0, vy.ptr(), vy.ld, coef.ptr(), bmom.ptr(), dw.ptr(), db.ptr(), N, HW, C, nseg, 1,
                                          0.0, 0, ws.ptr(), claim, None)
        torch.cuda.synchronize()
        what = f'batchnorm_moments_bwd {shape} ws {claim}/{full}'
        if claim < full:
            assert rc == PG_EWORKSPACE, (what, rc)
            for g in (bmom, dw, db, ws):
                G.assert_untouched(g, None, what)
        else:
            assert rc == PG_OK, (what, rc)
            assert B._rel(dw.inner(torch.float32), wt.grad) <= 5e-5 and B._rel(db.inner(torch.float32), bs.grad) <= 5e-5, what
            G.assert_untouched(bmom, 'all', what + ' mom'), G.assert_untouched(dw, 'all', what + ' dweight')
            G.assert_untouched(db, 'all', what + ' dbias'), G.assert_untouched(ws, claim, what + ' workspace')
        ins.check(what)
    ins.add(bmom, 'bmom')
    for claim in (full - 256, full):
        vd, gd = G.view(N, H, W, C, ld=C + 4, off=4)
        ws = G.flat(full, back=max(full, G.BACK))
        rc = lib.pg_batchnorm_bwd_apply(vg.ptr(), vg.ld, None, 0, vy.ptr(), vy.ld, coef.ptr(), bmom.ptr(), count, vd.ptr(), vd.ld, N, HW, C, nseg,
                                        1, 0.0, 0, ws.ptr(), claim, None)
        torch.cuda.synchronize()
        what = f'batchnorm_bwd_apply {shape} ws {claim}/{full}'
        if claim < full:
            assert rc == PG_EWORKSPACE, (what, rc)
            G.assert_untouched(gd, None, what), G.assert_untouched(ws, None, what)
        else:
            assert rc == PG_OK, (what, rc)
            assert B._rel(G.read_nchw(vd), y.grad) <= 5e-5, what
            G.assert_untouched(gd, 'slice', what + ' dy'), G.assert_untouched(ws, claim, what + ' workspace')
        ins.check(what)


# ------------------------------------------------------------------------------------------------ one process, no group
def _small(norm_layer, seed=3):
    """tests/test_batchnorm_gpu.py's _small_bn with the norm layer of choice."""
    import patchgan_amd as pg
    torch.manual_seed(seed)
    g = pg.UNet(3, 1, 4, norm_layer=norm_layer, activation='leakyrelu', final_act='sigmoid').to(DEV)
    d = pg.Discriminator(4, 4, n_layers=3, norm=True, norm_layer=norm_layer).to(DEV)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 256, 256, generator=gen)
    y = (torch.rand(2, 1, 256, 256, generator=gen) > 0.7).float()
    return g, d, x, y


def test_without_a_group_a_syncbatchnorm_pair_is_the_batchnorm_pair_bit_for_bit(tmp_path):
    runs = []
    for kind in (nn.BatchNorm2d, nn.SyncBatchNorm):
        g, d, x, y = _small(kind)
        t = B._trainer(g, d, tmp_path / kind.__name__, 'tversky')
        losses = [dict(t.batch(x, y, train=True)) for _ in range(3)]
        t.flush()
        torch.cuda.synchronize()
        runs.append((losses, g.flat.clone(), d.flat.clone(), g.bn_bufs.clone(), d.bn_bufs.clone(), g.bn_counters.clone(),
                     d.bn_counters.clone()))
    a, b = runs
    assert a[0] == b[0]
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)
    assert int(a[5][0]) == 3 and int(a[6][0]) == 9


# ------------------------------------------------------------------------------------------------ data parallel
def _collect(q, procs, timeout=300.0):
    """tests/test_dp_gpu.py's loop: one result per worker; fails at once when a worker died and leaves no rank behind on the GPU."""
    import queue
    import time
    out, t0 = [], time.monotonic()
    try:
        while len(out) < len(procs):
            try:
                out.append(q.get(timeout=1.0))
                continue
            except queue.Empty:
                pass
            dead = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
            assert not dead, f'worker(s) died (rank, exit code): {dead}'
            assert time.monotonic() - t0 < timeout, 'workers still running after the timeout'
    except BaseException:
        for p in procs:
            if p.is_alive():
                p.kill()
        raise
    return sorted(out, key=lambda r: r[0])


def _spawn(target, world, *args):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def _init_group(rank, world, port, backend):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    if backend == 'nccl':
        os.environ['PATCHGAN_DP_FORCE'] = '1'          # a one-rank RCCL group with the data-parallel path on
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(4)
    return dist


def _np(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def _fixture_worker(rank, world, port, q, name, nsteps, backend):
    dist = _init_group(rank, world, port, backend)
    try:
        import tempfile
        import patchgan_amd as pg
        from patchgan_amd.parallel import current, shard_batch
        gold = B.BNGolden(name)
        c = gold.cfg
        torch.manual_seed(gold.model_seed)
        g = pg.UNet(c['in_nc'], c['out_nc'], c['nf'], norm_layer=nn.SyncBatchNorm, use_dropout=False, activation=c['activation'],
                    final_act=c['final_act']).to(DEV)
        d = pg.Discriminator(c['in_nc'] + c['out_nc'], c['ndf'], n_layers=c['n_layers'], norm=c['norm'], norm_layer=nn.SyncBatchNorm).to(DEV)
        t = B._trainer(g, d, tempfile.mkdtemp(), c['loss_type'])
        t.bucket_bytes = 64 << 10          # several buckets even for the nf = 4 generator
        g.train()
        d.train()
        x, y = gold.inputs()
        xs, ys = shard_batch(x, y, rank, world)
        curve, step1 = [], None
        for s in range(nsteps):
            l = t.batch(xs, ys, train=True)
            curve.append([l[k] for k in LOSS_KEYS])
            if s == 0:
                t.flush()
                torch.cuda.synchronize()
                step1 = (_np({k: p.grad for k, p in g.named_parameters()}), _np({k: p.grad for k, p in d.named_parameters()}),
                         _np(g.state_dict()), _np(d.state_dict()))
        t.flush()
        torch.cuda.synchronize()
        state = (g.flat.cpu().numpy(), d.flat.cpu().numpy(), g.bn_bufs.cpu().numpy(), d.bn_bufs.cpu().numpy(),
                 g.bn_counters.cpu().numpy(), d.bn_counters.cpu().numpy())
        q.put((rank, np.array(curve), state, step1, (current().on, t.launch_mode)))
    finally:
        dist.destroy_process_group()


class _Dict:
    def __init__(self, d):
        self.d = {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}

    def state_dict(self):
        return self.d


def _check_against_fixture(name, res, nsteps, probes=True):
    gold = B.BNGolden(name)
    curve = res[0][1]
    want, want64 = gold.z['losses'][:nsteps], gold.z['losses64'][:nsteps]
    e_ref = np.maximum.accumulate(np.abs(want - want64).max(1))
    bound = np.maximum(1e-4, 4 * e_ref)
    err = np.abs(curve - want).max(1)
    print(name, 'loss error / max(1e-4, 4 e_ref(step)) per step', np.round(err / bound, 3), 'error', err, 'e_ref', e_ref)
    report = [('losses', 'per step', (err / bound).tolist())]
    if probes:
        gg, dg, gs, ds = res[0][3]
        B._check_probes(gold, 'ggrad1', 'ggrad1_64', _Dict(gg), 2e-4, report)
        B._check_probes(gold, 'dgrad1', 'dgrad1_64', _Dict(dg), 2e-4, report)
        B._check_probes(gold, 'run1/g', 'run1_64/g', _Dict(gs), 2e-4, report)       # (the counters exactly: 1 and 3 after one step)
        B._check_probes(gold, 'run1/d', 'run1_64/d', _Dict(ds), 2e-4, report)
        assert all(int(v) == 1 for k, v in gs.items() if k.endswith('num_batches_tracked'))
        assert all(int(v) == 3 for k, v in ds.items() if k.endswith('num_batches_tracked'))
    bad = [e for e in report if (max(e[2]) if isinstance(e[2], list) else e[2]) > 1.0]
    print(name, 'error / bound above 1:', bad, 'worst:', max(report, key=lambda e: max(e[2]) if isinstance(e[2], list) else e[2]))
    assert not bad, bad


@pytest.mark.parametrize('name', ['bn_a', 'bn_b', 'bn_c'])
def test_two_ranks_train_like_the_reference_on_the_whole_batch(name):
    """Two ranks over gloo on the one GPU, each on half of the fixture's batch (bn_b, bn_c: ONE sample per rank; bn_c at 128 x 128: a
    1 x 1 bottleneck, local count 1, global count 2), 5 steps, several gradient buckets.  Both ranks end bit-identical (weights,
    running statistics, counters) and report equal losses; against the fixture -- the reference's BatchNorm2d on the full batch --
    the loss curve per step within max(1e-4, 4 e_ref(step)), and after step 1 the all-reduced gradients and the running statistics
    within max(2e-4, 4 x the reference's own fp32-vs-float64 distance): what a BatchNorm weight gradient counted twice or an unbiased
    variance taken with the local count would miss."""
    nsteps = 5
    res = _spawn(_fixture_worker, 2, name, nsteps, 'gloo')
    (_, c0, s0, _, m0), (_, c1, s1, _, m1) = res
    assert m0 == (True, 'eager1') and m1 == (True, 'eager1')
    for u, v in zip(s0, s1):
        assert np.array_equal(u, v)
    assert np.array_equal(c0, c1)
    assert (s0[4] == nsteps).all()
    if B.BNGolden(name).cfg['norm']:
        assert (s0[5] == 3 * nsteps).all()
    _check_against_fixture(name, res, nsteps)


def test_one_rank_rccl_group_runs_the_split_path():
    """A one-rank RCCL group with PATCHGAN_DP_FORCE=1: the split path and the comm-stream ordering under the real backend."""
    nsteps = 3
    res = _spawn(_fixture_worker, 1, 'bn_a', nsteps, 'nccl')
    assert res[0][4] == (True, 'eager1')
    _check_against_fixture('bn_a', res, nsteps)


def _autograd_worker(rank, world, port, q):
    dist = _init_group(rank, world, port, 'gloo')
    try:
        from patchgan_amd.parallel import shard_batch
        g, d, x, y = _small(nn.SyncBatchNorm)
        xs, _ = shard_batch(x, y, rank, world)
        g.zero_grad()
        g(xs.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        q.put((rank, _np({k: p.grad for k, p in g.named_parameters()}),
               int(g.state_dict()['encoder.0.model.DownNorm0.num_batches_tracked']), _np(dict(g.named_buffers()))))
    finally:
        dist.destroy_process_group()


def test_autograd_path_synchronises_too():
    """g(x_half).sum().backward() on each of two ranks: the SUM of the ranks' parameter gradients is the single-process BatchNorm2d
    network's gradient on the whole batch (2e-4: the bound of test_autograd_path_matches_the_trainer_gradients); one
    running-statistics update on each rank, the same on both."""
    g, d, x, y = _small(nn.BatchNorm2d)
    g.zero_grad()
    g(x.to(DEV)).sum().backward()
    want = {k: p.grad.detach().clone() for k, p in g.named_parameters()}
    torch.cuda.synchronize()
    res = _spawn(_autograd_worker, 2)
    (_, g0, n0, b0), (_, g1, n1, b1) = res
    assert n0 == 1 and n1 == 1
    for k in b0:
        assert np.array_equal(b0[k], b1[k]), k
    for k, w in want.items():
        got = torch.from_numpy(g0[k]).double() + torch.from_numpy(g1[k]).double()
        assert B._rel(got, w) < 2e-4, (k, B._rel(got, w))
    assert want['encoder.3.model.DownNorm3.weight'].abs().sum() > 0
