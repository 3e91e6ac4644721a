"""The references, tolerances, inputs and case table of tests/test_bnkernels_gpu.py discriminate, shown without a GPU: the float64
reference is torch's batch_norm under float64 autograd (training and evaluation mode, one and two segments), the comparator accepts a
plain fp32 evaluation of every case in either summation order and rejects every seeded mutation of it where that mutation can show,
the knife-edge condition of the inputs holds, and every row reaches the kernel path it names (the launch plan of batchnorm.hip
mirrored on the host, tied to the library's own workspace query)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bn_util as B
from tests import normact_util as U

ALL = B.cases()
SMALL = [c for c in ALL if not c.large]
BY = {c.name: c for c in ALL}
ids = lambda cs: [c.name for c in cs]
TORCH_ACT = {'none': lambda t: t, 'leaky': lambda t: F.leaky_relu(t, 0.2), 'relu': F.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return B.inputs(BY[name])


# ---- the table reaches what it says -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ALL, ids=ids(ALL))
def test_case_reaches_its_path(case):
    for entry in ('act_fwd', 'act_bwd'):
        pl = B.bn_path(case, entry)
        flags = tuple(f for f, on in (('overhang', pl['overhang']), ('ragged', pl['ragged']),
                                      ('unrolled', pl['unrolled_partial'])) if on)
        assert (pl['path'], pl['vec'], flags) == (case.path, case.vec, case.flags), (case.name, entry, pl)
        assert pl['unrolled_apply'] or 'unrolled' not in flags
    # the entry points without a one-kernel form: the statistics pass always runs k_bn_partial, the apply passes k_bn_apply
    form = case.path if case.path != 'one-wg' else None
    for entry in ('stats', 'act_apply', 'bwd_apply'):
        pl = B.bn_path(case, entry)
        assert pl['path'] in ('chunked-fixed', 'chunked-flat') and pl['vec'] == case.vec and (form is None or pl['path'] == form)
    for entry in ('moments_fwd', 'moments_bwd'):
        assert B.bn_path(case, entry)['path'] == case.path


def test_plan_numbers_of_the_table():
    p = lambda name, entry='act_fwd': B.bn_path(BY[name], entry)
    assert [(p(n)['G'], p(n)['groups']) for n in ('16x516x3x3', '16x129x3x3-mis')] == [(2, 65), (2, 65)]
    assert [(p(n)['G'], p(n)['groups']) for n in ('2x512x1x1', '4x512x1x1')] == [(2, 64), (2, 64)]
    assert all(p(c.name)['G'] == 1 for c in ALL if c.path == 'one-wg' and p(c.name)['units'] < 127)
    assert (p('2x4x16x32')['path'], B.bn_plan(2, 512, 4, 4)['nchunk'], B.bn_plan(2, 512, 8, 4)['nchunk']) == ('one-wg', 1, 2)
    assert (p('2x64x24x24')['nchunk'], p('2x64x24x24')['ppc']) == (18, 32)
    assert (p('2x64x23x25')['nchunk'], p('2x64x23x25')['ppc'], 575 - 16 * 34) == (17, 34, 31)
    assert (p('2x4x32x33')['G'], p('2x4x32x33')['nchunk']) == (1, 2)
    assert (p('2x1x40x41')['units'], p('2x1x40x41')['nchunk'], p('2x1x40x41')['ppc']) == (1, 3, 547)
    assert (p('2x12x23x25')['units'], p('2x12x23x25-mis')['units'], p('2x6x23x25')['units'], p('2x260x23x25-mis')['units']) == (3, 12, 6, 260)
    big = p('8x512x32x33')
    assert (big['nchunk'], big['ppc'], 256 // big['G'], 1056 - 62 * 17) == (63, 17, 4, 2)
    # the unrolled main loop of k_bn_partial needs more than three pixels per lane and chunk: the large row alone; the fixed apply's
    # runs wherever a thread walks four pixels (2x64x24x24: 9 blocks of 16 pixel lanes, step 144 < 576 / 3)
    assert not any(p(c.name, e)['unrolled_partial'] for c in SMALL for e in B.ENTRIES)
    assert p('2x64x24x24')['unrolled_apply'] and not p('2x12x23x25')['unrolled_apply'] and big['unrolled_apply']
    # the split form's ranks hold one sample each: the rows of tests/test_bnkernels_gpu.py keep their paths at N = 1
    for name in ('2x8x4x4', '2x8x4x4-mis', '2x64x24x24', '2x4x64x65-mis', '2x12x23x25', '2x12x23x25-mis'):
        for e in ('moments_fwd', 'moments_bwd'):
            assert B.bn_path(BY[name], e, N=1)['path'] == BY[name].path, (name, e)


def test_workspace_mirror_is_the_librarys():
    """The host-side mirror of bn_plan that the path claims rest on answers pg_batchnorm_workspace_bytes for every case and a sweep,
    fewer than four channels on a chunked plane (no VEC 4 plan exists there) and the refused geometries included."""
    from patchgan_amd import _lib as L
    lib = L.load()
    for c in ALL:
        N, C, H, W = c.shape
        for nseg in (1, 2):
            assert int(lib.pg_batchnorm_workspace_bytes(N, H * W, C, nseg)) == B.workspace_bytes(N, H * W, C, nseg), (c.name, nseg)
    for N in (1, 2, 3, 16, 64):
        for HW in (1, 2, 511, 512, 513, 575, 4096, 100000):
            for C in (1, 2, 3, 4, 6, 24, 64, 260, 512, 1028):
                for nseg in (1, 2, 3):
                    want = B.workspace_bytes(N, HW, C, nseg)
                    assert int(lib.pg_batchnorm_workspace_bytes(N, HW, C, nseg)) == want, (N, HW, C, nseg)
                    assert (want == 0) == (nseg == 3 or N % nseg != 0)
    assert int(lib.pg_batchnorm_workspace_bytes(65536, 4, 4, 1)) == 0 and int(lib.pg_batchnorm_workspace_bytes(0, 4, 4, 1)) == 0


# ---- references ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SMALL, ids=ids(SMALL))
def test_reference_is_float64_autograd(case):
    """bn_ref against torch.nn.functional.batch_norm + autograd in float64: out, dy, dweight, dbias, and the batch statistics through
    torch's own running update (momentum 1: the running buffers ARE the batch mean and the unbiased variance)."""
    N, C, H, W = case.shape
    inp = _inputs(case.name)
    nchw = lambda t: t.reshape(N, H, W, C).permute(0, 3, 1, 2)
    seed = B.seed_of(case)
    worst = 0.0
    rel = lambda got, want: float((got - want).abs().max() / want.abs().max().clamp_min(1.0))
    for train, nseg in B.modes(case):
        for act, p, g2on in B.combos(case):
            ref, _ = B.evaluate(case, inp, train, nseg, act, p, g2on)
            x = nchw(inp['y']).clone().requires_grad_(True)
            w, b = inp['w'].clone().requires_grad_(True), inp['b'].clone().requires_grad_(True)
            if train:
                rms, rvs = torch.zeros(nseg, C, dtype=torch.float64), torch.zeros(nseg, C, dtype=torch.float64)
                z = torch.cat([F.batch_norm(xs, rms[s], rvs[s], w, b, True, 1.0, B.EPS) for s, xs in enumerate(x.split(N // nseg))])
                worst = max(worst, rel(ref['bstat'][..., 0], rms), rel(ref['bstat'][..., 1], rvs))
            else:
                z = F.batch_norm(x, inp['rm'].clone(), inp['rv'].clone(), w, b, False, 0.1, B.EPS)
            out = TORCH_ACT[act](z) * nchw(ref['keep']) * ref['ks']
            out.backward(nchw(inp['g1'] + inp['g2'] if g2on else inp['g1']))
            for got, want in ((nchw(ref['out']), out.detach()), (nchw(ref['dy']), x.grad), (ref['dweight'], w.grad), (ref['dbias'], b.grad)):
                worst = max(worst, rel(got, want))
    print(case.name, 'reference vs autograd', worst)
    assert worst <= 1e-12 and B.EPS == float(torch.tensor(1e-5, dtype=torch.float32))      # eps: the float the kernels take


def test_running_reference():
    """running_ref is torch's own update applied slot by slot (fp32 buffers, float64 batch statistics rounded as torch rounds)."""
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(4, 5, 3, 3, generator=gen, dtype=torch.float64) * 2 + 1
    rm0, rv0 = torch.randn(5, generator=gen), torch.rand(5, generator=gen) + 0.5
    bstat = torch.stack([torch.stack([xs.mean((0, 2, 3)), xs.var((0, 2, 3), unbiased=True)], -1) for xs in x.split(2)])
    rm, rv = B.running_ref(bstat, rm0, rv0)
    tm, tv = rm0.double().clone(), rv0.double().clone()
    for xs in x.split(2):
        F.batch_norm(xs, tm, tv, None, None, True, B.MOMENTUM, 1e-5)
        tm, tv = tm.float().double(), tv.float().double()
    assert B.running_ratio(tm, tv, rm, rv) <= 1.0
    assert B.running_ratio(rm + 2 * B.EPS32 * rm.abs(), rv, rm, rv) > 1.0


# ---- the comparator accepts correct fp32 and rejects the mutations --------------------------------------------------------------------

@pytest.mark.parametrize('case', ALL, ids=ids(ALL))
def test_comparator_accepts_plain_fp32(case):
    """Both summation orders, every mode and option of the row, without the chunked path's K term (a two-pass evaluation needs none
    of it): every ratio at most 1.  With K granted the fp64 batch variance is held to 2^-47 (var + mean^2), which presumes sums about
    32 additions deep: torch's blocked sum meets it too, the strictly sequential reverse order (M additions deep) is not asked to."""
    inp = _inputs(case.name)
    worst = {}
    for train, nseg in B.modes(case):
        for act, p, g2on in B.combos(case):
            ref, plain = B.evaluate(case, inp, train, nseg, act, p, g2on)
            _, rev = B.evaluate(case, inp, train, nseg, act, p, g2on, reverse=True)
            for res, chunked in ((plain, False), (rev, False), (plain, True)):
                for k, v in B.ratios(ref, plain, res, chunked).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(case.name, 'plain fp32 worst ratios', {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _applies(mut, case, train, nseg):
    """Where a mutation can show: the two-segment ones at nseg = 2, the evaluation-mode one there, the statistics ones in training
    mode on a plane of more than one pixel."""
    N, C, H, W = case.shape
    if mut in ('seg2_stats_of_seg1', 'whole_batch_stats', 'mask_no_seg_offset', 'dweight_one_segment', 'shift_other_segment_mean'):
        return train and nseg == 2
    if mut == 'eval_subtracts_mean':
        return not train
    if mut in ('stats_first_chunk', 'ragged_last_pixel'):
        return train and H * W > 1
    if mut == 'biased_bstat':
        return train
    return True


PAIRS = [(m, c) for m in B.MUTATIONS for c in ALL if any(_applies(m, c, t, s) for t, s in B.modes(c))]


@pytest.mark.parametrize('mut,case', PAIRS, ids=[f'{m}-{c.name}' for m, c in PAIRS])
def test_comparator_rejects_mutation(mut, case):
    """Dropout mutations at p = 0.2, the g2 mutation with a g2 (every row has both), in every mode of the row where the mutation can
    show; with the chunked path's K term granted (the wider of the two bounds)."""
    assert 0.2 in case.ps and True in case.g2s
    act = 'leaky' if 'leaky' in case.acts else case.acts[0]
    inp = _inputs(case.name)
    ran = 0
    for train, nseg in B.modes(case):
        if not _applies(mut, case, train, nseg):
            continue
        ref, plain = B.evaluate(case, inp, train, nseg, act, 0.2, True)
        _, bad = B.evaluate(case, inp, train, nseg, act, 0.2, True, mut=mut)
        r = B.ratios(ref, plain, bad, True)
        print(case.name, case.path, mut, 'train' if train else 'eval', nseg, {k: (round(v, 2) if math.isfinite(v) else v) for k, v in r.items()})
        assert max(r.values()) > 1.0, (train, nseg, r)
        ran += 1
    assert ran


def test_every_mutation_runs_somewhere():
    """Each of the thirteen mutations on at least one one-workgroup, one fixed and one flat row."""
    for mut in B.MUTATIONS:
        assert {'one-wg', 'chunked-fixed', 'chunked-flat'} <= {c.path for m, c in PAIRS if m == mut}, mut
    assert len(B.MUTATIONS) == 13


@pytest.mark.parametrize('case', ALL, ids=ids(ALL))
def test_knife_edge_condition(case):
    inp = _inputs(case.name)
    print(case.name, 'nudged fraction', inp['frac'])
    assert inp['left'] == 0 and inp['frac'] <= 0.01
    for k in ('y', 'g1', 'g2', 'w', 'b', 'rm', 'rv'):
        assert torch.equal(inp[k], inp[k].float().double()), k                  # representable in fp32
    for train, nseg in B.modes(case):
        z, thr, _ = B._z_of(inp['y'], inp['w'], inp['b'], nseg, train, inp['rm'], inp['rv'])
        live = (inp['w'] != 0).view(1, 1, -1).expand_as(z).clone()
        if case.const_ch is not None:
            live[..., case.const_ch] = False
            # the constant channel: z is the bias, or within the forward tolerance of it; never near 0
            assert float((z[..., case.const_ch] - inp['b'][case.const_ch]).abs().max()) <= 1e-9 * (1 if case.const_val == 0 else 1e6) or not train
            assert abs(float(inp['b'][case.const_ch])) >= 0.05
        assert not bool(((z.abs() < thr) & live).any()), (train, nseg)
    if case.const_ch is not None:
        assert bool((inp['y'][..., case.const_ch] == case.const_val).all()) and float(inp['w'][case.const_ch]) != 0
    if case.shape[1] >= 4:
        assert float(inp['w'][0]) < 0 and float(inp['w'][1]) == 0
