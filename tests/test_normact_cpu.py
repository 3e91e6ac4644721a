"""The references, tolerances and inputs of tests/test_normact_gpu.py discriminate, shown without a GPU: the float64 references are
float64 autograd, the mask port keeps at the stated rate, the comparator accepts a plain fp32 evaluation of every case with a factor
of two to spare (in either summation order) and rejects every seeded mutation of it, the knife-edge condition of the inputs holds,
and the table's cases reach the kernel paths its docstring names (the launch plan of norm_act.hip mirrored on the host)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import patchgan_oracle as O
from tests import normact_util as U

SMALL = [c for c in U.norm_cases() if not c.large]
ALL = U.norm_cases()
ids = lambda cs: [c.name for c in cs]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = {c.name: c for c in ALL + U.const_cases()}[name]
    return U.norm_inputs(case)


@functools.lru_cache(maxsize=None)
def _eval(name, act, p, g2on):
    case = {c.name: c for c in ALL + U.const_cases()}[name]
    y, g1, g2, _, _ = _inputs(name)
    g2 = g2 if g2on else None
    ref = U.norm_ref(y, g1, g2, act, p, U.seed_of(case))
    plain = U.plain_norm(y, g1, g2, act, p, U.seed_of(case))
    return case, (y, g1, g2), ref, plain


def _store(case, res):
    by, bo, bg, bd = U.MIX[case.mix]
    out, stats, dy = res
    return U.stored(out, bo), stats, U.stored(dy, bd)


# ---- the table reaches what it says -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ALL + U.const_cases(), ids=ids(ALL + U.const_cases()))
def test_case_reaches_its_path(case):
    for bwd in (False, True):
        pl = U.norm_plan(case, bwd)
        assert (pl['vec'], pl['path']) == (case.vec, case.path), (case.name, bwd, pl)


def test_plan_numbers_of_the_docstring_table():
    by = {c.name: c for c in ALL}
    for name in ('16x520x3x3', '16x130x3x3'):
        pl = U.norm_plan(by[name])
        assert (pl['G'], pl['groups'], pl['overhang']) == (4, 33, True), pl
    for c in ALL:
        if c.name not in ('16x520x3x3', '16x130x3x3') and c.path == 'one-wg':
            assert U.norm_plan(c)['G'] == 1, c.name
    assert (U.norm_plan(by['2x8x16x32'])['nchunk'], U.norm_plan(by['2x16x16x32-bf16'])['nchunk']) == (2, 2)
    pl = U.norm_plan(by['2x64x23x23'])
    assert (pl['nchunk'], pl['ppc'], 529 - 15 * pl['ppc']) == (16, 34, 19)                    # ragged last chunk
    assert (U.norm_plan(by['2x24x23x23'])['overhang'], U.norm_plan(by['2x24x23x23-bf16'])['overhang']) == (True, True)
    # the unrolled main loop of k_in_partial needs 4 pixels per lane and chunk; every other case stays in the tail loop
    big = {n: U.norm_plan(by[n]) for n in ('8x256x64x66', '8x256x64x66-bf16', '8x256x64x66-mis')}
    assert [(p['nchunk'], p['ppc'], p['ppl']) for p in big.values()] == [(128, 33, 8.25), (128, 33, 4.125), (32, 132, 33.0)]
    assert all(U.norm_plan(c)['ppl'] < 4 for c in SMALL if c.path != 'one-wg')
    # k_in_merge: 128 chunks = four full 32-wide blocks; the parts test adds 1, 5 and 33
    assert 8 * 256 * 4224 == 8650752


def test_workspace_mirror_is_the_librarys():
    """The host-side mirror of chunk_plan that the path claims rest on answers pg_instnorm_workspace_bytes for every case."""
    from patchgan_amd import _lib as L
    lib = L.load()
    for c in ALL + U.const_cases():
        N, C, H, W = c.shape
        assert int(lib.pg_instnorm_workspace_bytes(N, H * W, C)) == U.workspace_bytes(N, H * W, C), c.name
    for N, HW, C in ((1, 512, 4), (16, 64 * 64, 512), (1, 256 * 256, 64), (3, 511, 8), (2, 100000, 24), (64, 1024, 1)):
        assert int(lib.pg_instnorm_workspace_bytes(N, HW, C)) == U.workspace_bytes(N, HW, C), (N, HW, C)


def test_rne_bf16():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8 - 2.0 ** -40,
                      0.0, 3.0e-39], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -1.0 - 2.0 ** -7, 0.0, float(torch.tensor(3.0e-39).bfloat16())], dtype=torch.float64)
    assert torch.equal(U.rne_bf16(x), want)
    r = torch.randn(4096, dtype=torch.float64)
    assert torch.equal(U.rne_bf16(r.float().double()), r.float().bfloat16().double())
    s = torch.sort(r).values
    assert bool((U.rne_bf16(s)[1:] >= U.rne_bf16(s)[:-1]).all())


# ---- references ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SMALL, ids=ids(SMALL))
def test_references_are_float64_autograd(case):
    N, C, H, W = case.shape
    y, g1, g2, _, _ = _inputs(case.name)
    nchw = lambda t: t.view(N, H, W, C).permute(0, 3, 1, 2)
    worst = 0.0
    for act, p, g2on in U.combos(case):
        ref = U.norm_ref(y, g1, g2 if g2on else None, act, p, U.seed_of(case), eps=1e-5)
        x = nchw(y).clone().requires_grad_(True)
        out = O.apply_act(O.instance_norm(x), U.ORACLE_ACT[act]) * nchw(ref['keep']) * ref['ks']
        out.backward(nchw(g1 + g2 if g2on else g1))
        for got, want in ((nchw(ref['out']), out.detach()), (nchw(ref['dy']), x.grad)):
            worst = max(worst, float((got - want).abs().max() / want.abs().max().clamp_min(1.0)))
    print(case.name, 'reference vs autograd', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('act', U.ACTS)
def test_act_and_softmax_references_are_float64_autograd(act):
    y, g1, g2 = U.act_inputs(U.ACT_NPIX, 12, False)
    for p in (0.0, 0.2):
        x = y.clone().requires_grad_(True)
        m = U.mask_t(1, y.shape, p) * U.keep_scale(p)
        out = O.apply_act(x, U.ORACLE_ACT[act]) * m
        out.backward(g1 + g2)
        assert float((U.act_ref(y, act, p, 1) - out.detach()).abs().max()) <= 1e-12
        r = U.act_bwd_ref(g1, g2, out.detach(), act, p, 1)
        assert float((r['dy'] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    for C in U.SOFTMAX_CS:
        ys, h1, h2 = U.softmax_inputs(C)
        x = ys.clone().requires_grad_(True)
        o = torch.softmax(x, 1)
        o.backward(h1 + h2)
        assert float((U.softmax_ref(ys) - o.detach()).abs().max()) <= 1e-12
        assert float((U.softmax_bwd_ref(h1, h2, o.detach()) - x.grad).abs().max()) <= 1e-12


def test_keep_rate():
    worst = 0.0
    for seed in U.SEEDS:
        for p in (0.2, 0.5):
            for n in (100003, 2 * 529 * 64):
                k = U.keep_mask(seed, n, p)
                worst = max(worst, abs(k.mean() - (1 - p)) / (5 * math.sqrt(p * (1 - p) / n)))
    print('keep rate: worst fraction of the 5 sigma bound', worst)
    assert worst <= 1.0
    assert U.keep_mask(7, 1000, 0.0).all()
    # the stream is a function of (seed, element): a window of it is the same values
    assert np.array_equal(U.keep_mask(U.SEEDS[2], 50, 0.2, start=1000), U.keep_mask(U.SEEDS[2], 1050, 0.2)[1000:])


# ---- the comparator accepts correct fp32 and rejects the mutations --------------------------------------------------------------------

@pytest.mark.parametrize('case', SMALL + U.const_cases(), ids=ids(SMALL + U.const_cases()))
def test_comparator_accepts_plain_fp32(case):
    by, bo, bg, bd = U.MIX[case.mix]
    worst = {}
    for act, p, g2on in U.combos(case):
        _, (y, g1, g2), ref, plain = _eval(case.name, act, p, g2on)
        rev = U.plain_norm(y, g1, g2, act, p, U.seed_of(case), reverse=True)
        for res in (plain, rev):
            fp = case._replace(mix='fp32')
            r = U.norm_ratios(fp, ref, plain[2], res[0].double(), res[1], res[2].double())
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if bo or bd:            # ... and what a bf16 store of it leaves lies in the interval
                rb = U.norm_ratios(case, ref, plain[2], *_store(case, res))
                assert rb['fwd'] <= 1.0 and rb['bwd'] <= 1.0, (case.name, act, p, g2on, rb)
    print(case.name, 'plain fp32 worst ratios', {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


def _applies(mut, case):
    if mut in ('last_unit_neighbour_stats',):
        return case.shape[1] >= 2
    return True


@pytest.mark.parametrize('case', SMALL, ids=ids(SMALL))
@pytest.mark.parametrize('mut', U.NORM_MUTATIONS)
def test_comparator_rejects_norm_mutation(mut, case):
    """Dropout mutations at p = 0.2, the g2 mutation with a g2: each case of the table has both."""
    assert 0.2 in case.ps and True in case.g2s and _applies(mut, case)
    act = 'leaky' if 'leaky' in case.acts else case.acts[0]
    _, (y, g1, g2), ref, plain = _eval(case.name, act, 0.2, True)
    res = U.plain_norm(y, g1, g2, act, 0.2, U.seed_of(case), mut=mut)
    r = U.norm_ratios(case, ref, plain[2], *_store(case, res))
    print(case.name, case.path, mut, {k: (round(v, 2) if math.isfinite(v) else v) for k, v in r.items()})
    assert max(r.values()) > 1.0, r
    if mut == 'mask_bwd_transposed':
        assert r['fwd'] <= 1.0 < r['bwd']          # a forward that is right and a backward that is not


@pytest.mark.parametrize('case', ALL, ids=ids(ALL))
def test_knife_edge_condition(case):
    y, g1, g2, frac, left = U.norm_inputs(case) if case.large else _inputs(case.name)
    print(case.name, 'nudged fraction', frac)
    assert left == 0 and frac <= 0.01
    by, bo, bg, bd = U.MIX[case.mix]
    for t, bf in ((y, by), (g1, bg), (g2, bg)):
        assert torch.equal(t, U.stored(t, bf))                  # representable in the tensor's storage type


# ---- activation and softmax ---------------------------------------------------------------------------------------------------------

def _act_setup(C, mix, act, p, g2on, seed=1):
    bf = mix == 'bf16'
    y, g1, g2 = U.act_inputs(U.ACT_NPIX, C, bf)
    g2 = g2 if g2on else None
    ref = U.act_ref(y, act, p, seed)
    a = U.stored(ref, bf)                      # what the forward kernel stored: the backward's input
    return bf, y, g1, g2, ref, a, U.act_bwd_ref(g1, g2, a, act, p, seed)


@pytest.mark.parametrize('name,C,layout,mix,vec', U.ACT_CASES, ids=[c[0] for c in U.ACT_CASES])
def test_act_comparator(name, C, layout, mix, vec):
    assert U.vec_of(C, layout, (mix == 'bf16',) * 4) == vec
    worst = 0.0
    for act in U.ACTS:
        for p in (0.0, 0.2):
            for g2on in (False, True):
                bf, y, g1, g2, ref, a, rb = _act_setup(C, mix, act, p, g2on)
                wf = U.worst_ratio(U.plain_act(y, act, p, 1).double(), ref, U.tol_act_fwd(ref))
                wb = U.worst_ratio(U.plain_act_bwd(g1, g2, a, act, p, 1).double(), rb['dy'], U.tol_act_bwd(rb, act, p))
                worst = max(worst, wf, wb)
                assert U.worst_ratio(U.stored(U.plain_act(y, act, p, 1), bf), ref, U.tol_act_fwd(ref), bf) <= 1.0
                for mut in U.ACT_MUTATIONS:
                    if (mut in ('mask_off_by_one', 'no_keep_scale') and p == 0) or (mut == 'g2_dropped' and not g2on):
                        continue
                    if mut == 'grad_from_scaled_out' and (p == 0 or act not in ('tanh', 'sigmoid')):
                        continue
                    f = U.worst_ratio(U.stored(U.plain_act(y, act, p, 1, mut), bf), ref, U.tol_act_fwd(ref), bf)
                    b = U.worst_ratio(U.stored(U.plain_act_bwd(g1, g2, a, act, p, 1, mut), bf), rb['dy'], U.tol_act_bwd(rb, act, p), bf)
                    assert max(f, b) > 1.0, (name, act, p, g2on, mut, f, b)
    print(name, 'plain fp32 worst ratio', worst)
    assert worst <= 0.5


@pytest.mark.parametrize('C', U.SOFTMAX_CS)
def test_softmax_comparator(C):
    y, g1, g2 = U.softmax_inputs(C)
    ref = U.softmax_ref(y)
    o = ref.float().double()
    fwd = U.worst_ratio(U.plain_softmax(y).double(), ref, U.tol_softmax_fwd(y, ref))
    worst = 0.0
    for h2 in (None, g2):
        want = U.softmax_bwd_ref(g1, h2, o)
        worst = max(worst, U.worst_ratio(U.plain_softmax_bwd(g1, h2, o).double(), want, U.tol_softmax_bwd(g1, h2, o)))
        for mut in ('g2_dropped', 'last_pixel_nan'):
            if mut == 'g2_dropped' and (h2 is None or C == 1):          # (C = 1: the gradient is 0 whatever comes in)
                continue
            assert U.worst_ratio(U.plain_softmax_bwd(g1, h2, o, mut).double(), want, U.tol_softmax_bwd(g1, h2, o)) > 1.0, (C, mut)
    for mut in ('no_max_sub', 'last_pixel_nan'):
        assert U.worst_ratio(U.plain_softmax(y, mut).double(), ref, U.tol_softmax_fwd(y, ref)) > 1.0, (C, mut)
    print('softmax C =', C, 'plain fp32 worst ratio: forward', fwd, 'backward', worst)
    # the forward formula has no term for the C - 1 roundings of the sequential sum: at C = 32 the plain evaluation uses 0.86 of it
    # (0.45 and less for C <= 7), so the factor of two to spare holds up to C = 7 and for the backward only
    assert worst <= 0.5 and fwd <= (0.5 if C <= 7 else 1.0)
