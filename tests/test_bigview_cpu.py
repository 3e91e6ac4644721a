"""The host side of the large-view addressing tests (tests/bigview_util.py, tests/test_bigview_gpu.py): the stride chooser and its
sensitivity property, the torch scatter / gather helpers, the case lists against the planner, and the engine's size rule.  No GPU."""
import torch

from patchgan_amd import _lib as L
from tests import bigview_util as B
from tests import exact_util as X
import tests.test_bigview_gpu as G      # (registers the Part 2 views)


def test_limit_is_the_one_the_strides_are_built_on():
    assert B.limit() == 0x60000000 and B.limit() < B.TIER_START['S'] < B.TIER_START['W']


def test_closed_form_admissibility_is_the_literal_property():
    """`admissible` against the element-by-element statement, on strides that fail it in each of the four ways and on ones that pass."""
    P, C = 40, 8
    seen = set()
    for elem in (4, 2):
        for w in (1 << 31, 1 << 32):
            we = w // elem
            for k in (1, 3, 17, P + 5):
                for r in (0, C - 1, C, -1, -C, -C + 1, 12345):
                    ld = (we - r) // k if r >= 0 else (we + (-r)) // k
                    for cand in range(max(ld - 9, C), ld + 10):
                        a, b = B.admissible(P, cand, C, elem), B.admissible_literal(P, cand, C, elem)
                        assert a == b, (P, cand, C, elem)
                        seen.add(a)
    assert seen == {True, False}
    assert not B.admissible(P, 1 << 27, C, 4)           # a power of two: pixel p + 4 sits exactly 2^31 bytes after pixel p
    assert B.admissible(P, (1 << 27) + 8, C, 4)


def test_every_stride_of_both_parts_is_in_its_tier_and_admissible():
    lim = B.limit()
    views = B.all_views()
    assert len(views) > 60 and len(B.PART2_VIEWS) >= 30, (len(views), len(B.PART2_VIEWS))
    peak = {}
    for what, P, C, elem, tiers in views:
        lds = {}
        for tier in tiers:
            ld = lds[tier] = B.choose_ld(tier, P, C, elem, lim)
            g = 8 if elem == 2 else 4
            assert ld % g == 0 and ld >= C and (P - 1) * ld + C < 2 ** 31, (what, tier, ld)       # within 2^31 elements: in scope
            assert B.in_tier(tier, P, ld, C, elem, lim), (what, tier, ld)
            assert B.admissible_literal(P, ld, C, elem), (what, tier, ld)
            if tier in ('S', 'W'):      # literally: at least a quarter of the pixels start at or beyond the mark
                starts = [p * ld * elem for p in range(P)]
                assert 4 * sum(s >= B.TIER_START[tier] for s in starts) >= P, (what, tier, ld)
                assert B.extent(P, ld, C, elem) >= lim
            peak[tier] = max(peak.get(tier, 0), B.region_bytes(P, ld, elem))
        if 'B' in lds and 'A' in lds:   # the two strides straddle the limit as tightly as admissibility allows
            assert lds['B'] < lds['A'], what
            between = range(lds['B'] + g, lds['A'], g)
            assert all(not (B.extent(P, m, C, elem) < lim and B.admissible(P, m, C, elem) and (m - lds['B']) % 8 == 0) for m in between), what
            assert all(not (B.extent(P, m, C, elem) >= lim and B.admissible(P, m, C, elem) and (lds['A'] - m) % 8 == 0) for m in between), what
    print({t: f'{v / B.GIB:.3f} GiB' for t, v in peak.items()})
    assert max(peak.values()) <= B.MAX_ARENA == 8 * B.GIB
    assert max(peak[t] for t in 'BAS') <= B.MAX_ARENA_BAS


def test_scatter_and_gather_round_trip():
    """The torch helpers at a small ld on the CPU, fp32 and bf16: what is scattered is read back, lands where the engine View says
    it does, and the count sees exactly it."""
    N, H, W, C, ld, apron = 2, 3, 5, 6, 16, 64
    P = N * H * W
    for bf in (False, True):
        elem = 2 if bf else 4
        a = B.Arena(B.region_bytes(P, ld, elem, apron), 'cpu', apron)
        a.fill()
        assert a.count(a.nbytes, bf) == 0 and a.count(a.nbytes, not bf) == 0
        x = torch.arange(N * C * H * W, dtype=torch.float32).reshape(N, C, H, W) % 97
        a.pixels(P, ld, C, bf).copy_(B.to_pixels(x))
        assert a.count(a.nbytes, bf) == P * C
        assert torch.equal(B.from_pixels(a.pixels(P, ld, C, bf).float(), N, H, W), x)
        v = a.view(N, H, W, C, ld, bf)
        assert v.ptr() == a.t.data_ptr() + apron and (v.npix, v.ld, v.C, v.bf) == (P, ld, C, bf)
        flat = a.typed(bf)
        for n, c, h, w in ((0, 0, 0, 0), (1, 5, 2, 4), (1, 2, 0, 3)):
            assert float(flat[apron // elem + ((n * H + h) * W + w) * ld + c]) == float(x[n, c, h, w])
        assert bool(flat[:apron // elem].isnan().all()) and bool(a.pixels(P, ld, ld, bf)[:, C:].isnan().all())
    assert torch.equal(B.from_pixels(B.to_pixels(x), N, H, W), x)


def test_conv_case_lists_resolve_to_their_families():
    """Host-only planner queries: every family the issue names has a case for each of its ops, the case is on that family, and no
    candidate with fewer pixels is."""
    from patchgan_amd import engine as E
    cases = B.exact_cases()
    have = {(c.family, c.op) for c in cases}
    need = {(f, op) for f, ops in B.FAMILY_OPS.items() for op in ops}
    assert have == need, sorted(need - have)
    for c in cases:
        sym, split = E.ConvOp(*c.geom, c.algo).describe(c.op)
        assert (sym, split) == (c.sym, c.split) and B.family_of(sym) == c.family, c
        assert B.case_fits(c.geom, c.op), c
        X.budget_for(X.exact_operands(c.geom), c.op, sym)
        X.budget_for(X.exact_operands(c.geom), c.op, B.GENERIC[c.op])
        assert X.path_of(B.GENERIC[c.op], c.geom[5]) == 'gemm'
    for geom, algo in B.exact_candidates():
        for op in range(3):
            sym = E.ConvOp(*geom, algo).describe(op)[0]
            c = B.exact_case(B.family_of(sym), op)
            assert sum(B.pixels_of(c.geom)) <= sum(B.pixels_of(geom)) or not B.case_fits(geom, op), (c, geom)
    assert any(c.split > 1 for c in cases)          # split-K rides along
    for c in B.wino1_cases():
        sym = E.ConvOp(*c.geom, c.algo).describe(c.op)[0]
        assert sym == c.sym and B.case_fits(c.geom, c.op), (c, sym)
    fams = {c.family for c in B.bf16_cases()}
    assert fams == {'bf16x flat', 'bf16x ring', 'bf16r', 'wgrad_bf16x', 'ca1 bf16 big'}, fams
    for c in B.bf16_cases():
        X.budget_for(X.exact_operands(c.geom), c.op, c.sym)


def test_engine_extent_is_never_below_the_c_sides():
    """View.extent_bytes (npix * ld) >= tensor_bytes ((npix - 1) * ld + C) for the same view, so ConvOp.fits is the more
    conservative of the two rules: whatever the engine plans a hand-over for, the launch sees below the limit too."""
    from patchgan_amd import engine as E

    class Fake:
        def data_ptr(self):
            return 1 << 21
    lim = B.limit()
    for what, P, C, elem, tiers in B.all_views():
        for tier in tiers:
            ld = B.choose_ld(tier, P, C, elem, lim)
            v = E.View(Fake(), 0, ld, 1, 1, P, C, elem == 2)
            assert v.extent_bytes >= B.extent(P, ld, C, elem), (what, tier)
            if tier != 'B':
                assert not E.ConvOp.fits(v), (what, tier)
    for C, ld in ((1, 1), (3, 4), (64, 64), (64, 128)):
        for P in (1, 2, 1000):
            assert E.View(Fake(), 0, ld, 1, 1, P, C).extent_bytes >= B.extent(P, ld, C, 4)
