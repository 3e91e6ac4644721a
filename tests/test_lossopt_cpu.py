"""The references, tolerances and case tables of tests/test_lossopt_gpu.py discriminate, shown without a GPU: a plain fp32 evaluation of
every operation passes every tolerance on every case, each seeded mutation of it is rejected by the case and the check the tables
name for it, the float64 references agree with the oracle's loss expressions and torch's Adam, and the max-norm assertions of
test_seg_losses accept two of those mutations on that test's own inputs."""
import pytest
import torch

from oracle import patchgan_oracle as O
from tests import lossopt_util as U
from tests.normact_util import worst_ratio

ids = lambda cs: [c.name for c in cs]
CHAIN = U.chain_cases()


# ---- the plain evaluation is accepted ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', U.reduce_cases() + [U.FUSED_REMAINDER], ids=ids(U.reduce_cases() + [U.FUSED_REMAINDER]))
def test_plain_sums_pass(case):
    p, y = U.loss_inputs(case)
    S, A = U.sums_ref(p, y)
    r = worst_ratio(U.plain_sums(p, y), S, U.tol_sums(A, case.H * case.W))
    print(f'ratio plain sums {case.name} {r:.4f}')
    assert r <= 1.0
    assert U.loss_nsplit(case.N, case.H * case.W, case.C) == (case.nsplit, case.kernel == 'c4')


@pytest.mark.parametrize('mode', U.MODES)
@pytest.mark.parametrize('case', [c for c, _ in CHAIN], ids=[f'{c.name}-{lay}' for c, lay in CHAIN])
def test_plain_chain_passes(case, mode):
    r = U.chain_ratios(case, mode, U.plain_chain(case, mode))
    print(f'ratio plain chain {case.name} {mode} ' + ' '.join(f'{k}={v:.4f}' for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert U.loss_nsplit(case.N, case.H * case.W, case.C) == (case.nsplit, case.kernel == 'c4')


def test_plain_multitrip_gradient_passes():
    case = U.MULTITRIP
    r = U.chain_ratios(case, 'bce', U.plain_chain(case, 'bce'))
    assert max(r.values()) <= 1.0, r
    assert case.N * case.H * case.W > 8192 * 256 and U.loss_nsplit(case.N, case.H * case.W, case.C) == (case.nsplit, False)


@pytest.mark.parametrize('case', U.adam_cases() + [U.ADAM_BIG], ids=lambda c: f'n{c.n}-t{c.t}-lr{c.lr}-{"carried" if c.carried else "zero"}')
def test_plain_adam_passes(case):
    sc = U.adam_scalars(case.t, case.lr)
    ref, tol = U.adam_ref(U.adam_inputs(case), sc)
    r = U.adam_ratios(U.plain_adam(U.adam_inputs(case), sc), ref, tol)
    assert max(r.values()) <= 1.0, r


# ---- every mutation is rejected where the table says ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('mut', U.SUM_MUTATIONS + U.FIN_MUTATIONS + U.GRAD_MUTATIONS)
def test_chain_mutation_is_rejected(mut):
    case, mode, key = U.mutation_table()[mut]
    if key == 'sums':
        p, y = U.loss_inputs(case)
        S, A = U.sums_ref(p, y)
        assert worst_ratio(U.plain_sums(p, y), S, U.tol_sums(A, case.H * case.W)) <= 1.0
        r = worst_ratio(U.plain_sums(p, y, mut, case.nsplit), S, U.tol_sums(A, case.H * case.W))
    else:
        assert max(U.chain_ratios(case, mode, U.plain_chain(case, mode)).values()) <= 1.0
        r = U.chain_ratios(case, mode, U.plain_chain(case, mode, mut))[key]
    print(f'ratio mutation {mut} {case.name} {mode} {key} {r:.3g}')
    assert not r <= 1.0


@pytest.mark.parametrize('mut', U.ADAM_MUTATIONS)
def test_adam_mutation_is_rejected(mut):
    case, key = U.adam_mutation_table()[mut]
    sc = U.adam_scalars(case.t, case.lr)
    ref, tol = U.adam_ref(U.adam_inputs(case), sc)
    r = U.adam_ratios(U.plain_adam(U.adam_inputs(case), sc, mut), ref, tol)[key]
    print(f'ratio mutation {mut} n={case.n} {key} {r:.3g}')
    assert not r <= 1.0


def test_every_listed_mutation_has_a_case():
    assert set(U.mutation_table()) == set(U.SUM_MUTATIONS + U.FIN_MUTATIONS + U.GRAD_MUTATIONS)
    assert set(U.adam_mutation_table()) == set(U.ADAM_MUTATIONS)


# ---- the references are the oracle's ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode,name', [('tversky', 'tversky'), ('wbce', 'weighted_bce'), ('mae', 'MAE')])
def test_loss_reference_is_the_oracles_expression(mode, name):
    case = CHAIN[1][0]
    p, y = U.loss_inputs(case)
    nchw = lambda x: x.permute(0, 2, 1).reshape(case.N, case.C, case.H, case.W)
    want = O.seg_loss(name, nchw(p), nchw(y), 200)
    ref = U.chain_ref(case, mode)
    assert abs(float(ref['L']) - float(want)) <= 1e-6 * abs(float(want))         # (w in fp32 here, in float64 there)
    L, coef, _, _ = U.value_coef_ref(mode, ref['S'], ref['gsum2'], ref['B'], ref['HW'], ref['alpha'])
    assert abs(float(L) - float(ref['L'])) <= 1e-12 * abs(float(L))
    # the coefficients (autograd in S) reproduce the gradient (autograd in p) through the header's three gradient forms
    k0, k1 = coef[..., 0].unsqueeze(1), coef[..., 1].unsqueeze(1)
    g = k0 * y + k1 if mode == 'tversky' else k0 * torch.sign(p - y) if mode == 'mae' else k0 * (p - y) / ((1 - p) * p).clamp_min(U.CLAMP)
    assert worst_ratio(g, ref['g'], 1e-12 * ref['g'].abs() + 1e-300) <= 1.0


def test_adam_reference_is_torchs_step():
    case = U.AdamCase(1023, 3, 1e-3, True)
    p, g, m, v = U.adam_inputs(case)
    b1, b2, eps, lrbc1, sbc2 = U.adam_scalars(case.t, case.lr)
    (p1, m1, v1), _ = U.adam_ref((p, g, m, v), (b1, b2, eps, lrbc1, sbc2))
    q, mm, vv = p.clone(), m.clone(), v.clone()
    O.adam_update(q, g, mm, vv, case.t, case.lr)
    for a, b in ((p1, q), (m1, mm), (v1, vv)):
        # float32 scalars here, Python doubles there: 1 - fl32(0.999) is 0.0010000467, 4.7e-5 above torch's 0.001
        assert worst_ratio(a, b, 1e-4 * (b.abs() + (q - p).abs()) + 1e-300) <= 1.0


def test_pad_reference_rounds_to_nearest_even():
    src, want, sub, nan = U.pad_inputs(257, 7)
    assert int(nan.sum()) > 0 and int(sub.sum()) > 0 and set(b & 0xFFFFFFFF for b in src[:, :7].reshape(-1).tolist()) >= set(U.PAD_BITS)
    tor = src.view(torch.float32).bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF
    tor[:, 7:] = 0
    assert U.pad_mismatches(tor, want, torch.zeros_like(sub), nan) == 0      # torch's own RNE conversion, subnormals kept
    assert U.pad_mismatches(tor + 1, want, sub, nan) > 0 and bool((want[:, 7:] == 0).all())


# ---- what the max-norm assertions let through ------------------------------------------------------------------------------------------------

def _seg_losses_inputs(C):
    """The inputs of tests/test_kernels_gpu.py::test_seg_losses, as (N, HW, C) float64."""
    g = torch.Generator().manual_seed(5)
    N, H, W = 3, 32, 24
    p = torch.rand(N, C, H, W, generator=g).clamp(1e-4, 1 - 1e-4)
    y = (torch.rand(N, C, H, W, generator=g) > 0.7).float()
    f = lambda x: x.reshape(N, C, H * W).permute(0, 2, 1).contiguous().double()
    return f(p), f(y), N, H * W


def _rel_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def test_max_norm_passes_a_wrong_weight_on_a_light_plane():
    """Weighted BCE, C = 3, the inputs of test_seg_losses: rel_err < 2e-5 is 2e-5 of the tensor's largest gradient (259, median 0.05).
    It accepts (a) the weight of the lightest (n, c) plane built from a sum_hw y that is one pixel off, and (b) an error of 10 % on
    every element below the median; the per-element comparator rejects both."""
    p, y, N, HW = _seg_losses_inputs(3)
    L, g = U.grad_ref('wbce', p, y, 200.0)
    S, _ = U.sums_ref(p, y)
    gsum2 = U.prepare_ref(S)
    _, coef, _, _ = U.value_coef_ref('wbce', S, gsum2, N, HW, 200.0)
    tol = U.tol_grad('wbce', p, y, g, coef, U.coef_tol_for_grad('wbce', coef, 3, N, HW, 200.0))
    good = U.plain_grad('wbce', p, y, coef.float())
    n, c = divmod(int(g.abs().amax(1).argmin()), 3)
    S_bad = S.clone()
    S_bad[n, c, 1] += 1.0
    _, bad_coef = U.plain_finalize('wbce', S_bad, gsum2, N, HW, 200.0)
    bad_w = U.plain_grad('wbce', p, y, bad_coef)
    bad_small = torch.where(g.abs() <= g.abs().median(), good.double() * 1.1, good.double())
    print(f'max |g| {float(g.abs().max()):.1f} median {float(g.abs().median()):.3f} rel_err good {_rel_err(good, g):.2e} '
          f'one-pixel weight {_rel_err(bad_w, g):.2e} 10 % on the small half {_rel_err(bad_small, g):.2e}')
    assert _rel_err(good, g) < 2e-5 and worst_ratio(good, g, tol) <= 1.0
    assert _rel_err(bad_w, g) < 2e-5 and worst_ratio(bad_w, g, tol) > 100
    assert _rel_err(bad_small, g) < 2e-5 and worst_ratio(bad_small, g, tol) > 1e4


def test_bit_equality_of_two_forms_passes_a_stale_lane():
    """Tversky, C = 4: lane 3 of every pixel keeps its neighbour's value.  The staged and the one-launch form share loss_grad_pass, so
    the same defect sits in both and their bit-equality -- the only check the scalar-store form of the C = 4 path runs under -- holds;
    the per-element comparator rejects it.  (Where a max-norm test reaches the lane it sees this defect too: rel_err is 1.1.)"""
    p, y, N, HW = _seg_losses_inputs(4)
    L, g = U.grad_ref('tversky', p, y, 200.0)
    S, _ = U.sums_ref(p, y)
    _, coef, _, _ = U.value_coef_ref('tversky', S, U.prepare_ref(S), N, HW, 200.0)
    staged, fused = (U.plain_grad('tversky', p, y, coef.float(), 'stale_lane3') for _ in range(2))
    tol = U.tol_grad('tversky', p, y, g, coef, U.coef_tol_for_grad('tversky', coef, 4, N, HW, 200.0))
    assert torch.equal(staged, fused)
    assert worst_ratio(U.plain_grad('tversky', p, y, coef.float()), g, tol) <= 1.0 and worst_ratio(staged, g, tol) > 1e4
