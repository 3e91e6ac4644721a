"""Large-view addressing on the GPU: every kernel on a view whose byte offsets pass pg_conv_max_tensor_bytes(), 2^31 and 2^32.

The device, the stride tiers B / A / S / W, the admissibility of the strides and what is out of scope (views beyond 2^31 elements;
tier W of bf16 tensors is one) are described in tests/bigview_util.py.  After every call two things are checked: the result (Part 1:
the float64 convolution, zero tolerance, and bit-identity with the same call on compact views; Part 2: bit-identity with the same call
on compact views, which the existing tests hold to float64), and that the number of non-NaN elements of the arena -- apron, view and
gaps -- is exactly what the call was entitled to write there.

bf16 tensors (PG_IO_*) run in tier B and must be refused (PG_EINVAL, nothing written) in tiers A and S, as an input and as an output.
The image-facing kernels, whose ld is fixed by the 4- or 8-channel pixel, get real views of 10^8 pixels below and at the limit (the
last section).

Tiers B, A and S need at most 5 GiB and always run; tier W (8 GiB) is skipped only when torch.cuda.mem_get_info() shows too little
free memory.  Every test prints the family, the planner's symbol, and per tier the ld, the extent and the non-NaN count found against
expected."""
import ctypes
import time

import pytest
import torch

from patchgan_amd import _lib as L
from tests import bigview_util as B
from tests import exact_util as X

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
GROUPS = {'BAS': ('B', 'A', 'S'), 'W': ('W',)}
_ARENA = []


def _arena(tiers):
    """The module's one arena: 8 GiB where the device has them free, else the 5 GiB of tiers B, A and S."""
    if not _ARENA:
        free = torch.cuda.mem_get_info()[0]
        big = free >= B.MAX_ARENA + 2 * B.GIB
        _ARENA.append(B.Arena(B.MAX_ARENA if big else B.MAX_ARENA_BAS, DEV))
        _ARENA.append(None if big else f'tier W needs an {B.MAX_ARENA >> 30} GiB arena, torch.cuda.mem_get_info() shows {free / B.GIB:.1f} GiB free')
    if 'W' in tiers and _ARENA[1]:
        pytest.skip(_ARENA[1])
    return _ARENA[0]


@pytest.fixture(scope='module', autouse=True)
def _release_arena():
    """The arena lives for this module only: the tests that follow measure the device memory they use themselves."""
    yield
    from patchgan_amd import engine as E
    _ARENA.clear()
    E.release_workspaces()
    torch.cuda.empty_cache()


def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=DEV)


class _Compact:
    """A compact [P][C] operand in a NaN-filled buffer of its own (ld = C rounded up to the vector width), as an engine View."""

    def __init__(self, N, H, W, C, x=None, bf=False):
        from patchgan_amd import engine as E
        self.P, self.C, self.ld = N * H * W, C, B.compact_ld(C, bf)
        self.t = _nan(self.P * self.ld, torch.bfloat16 if bf else torch.float32)
        self.v = E.View(self.t, 0, self.ld, N, H, W, C, bf)
        if x is not None:
            self.pixels().copy_(B.to_pixels(x))

    def pixels(self):
        return self.t.view(self.P, self.ld)[:, :self.C]


def _line(what, tier, ld, ext, found, want):
    return f'  {what} tier {tier}: ld {ld} extent {ext} B ({ext / B.GIB:.3f} GiB) non-NaN {found} / {want}'


# ---- Part 1: convolutions -----------------------------------------------------------------------------------------------------------------
class _Conv:
    """One conv case: operands on the device, the compact call's result and, for the exact class, the float64 reference as fp32."""

    def __init__(self, case):
        from patchgan_amd import engine as E
        from tests import wino1_util as W1
        from tests.gpu_util import pack
        self.case, self.geom = case, case.geom
        N, Hb, Wb, Ca, Cb, s = case.geom
        Hs, Ws = X.dims(case.geom)
        self.shape = {'big': (N, Hb, Wb, Cb), 'small': (N, Hs, Ws, Ca)}
        self.bf = {'big': bool(getattr(case, 'io', 0) & L.IO_BIG_BF16), 'small': bool(getattr(case, 'io', 0) & L.IO_SMALL_BF16)}
        self.cpu = X.exact_operands(case.geom) if case.klass != 'wino1' else W1.normal_operands(case.geom)
        self.o = W1.on_device(self.cpu, DEV)
        self.pk = pack(self.o.Wt)
        self.cop = E.ConvOp(*case.geom, case.algo)
        self.ins, self.out = B.operand_shapes(case.geom, case.op)
        self.x = {'big': self.o.big, 'small': self.o.small}

    def compact(self, role, fill=True):
        return _Compact(*self.shape[role], self.x[role] if fill else None, self.bf[role])

    def launch(self, views):
        """The op on {'big': View, 'small': View}; returns the flat result of op 2 (dP then dbias), None otherwise."""
        o, op = self.o, self.case.op
        if op == 0:
            self.cop.big2small(views['big'], self.pk, 0, o.bias_a, 0, views['small'], L.ACT_NONE)
        elif op == 1:
            self.cop.small2big(views['small'], self.pk, 0, o.bias_b, 0, views['big'], L.ACT_NONE)
        else:
            N, Hb, Wb, Ca, Cb, s = self.geom
            dP, db = _nan(16 * Ca * Cb), _nan(Ca)
            self.dP = dP                        # (what a refused call must leave untouched)
            if self.case.klass == 'bf16':       # (the bf16 networks' convolutions that reach k_wgrad_bf16x have no bias)
                self.cop.wgrad(views['small'], views['big'], dP, 0)
                return dP
            self.cop.wgrad(views['small'], views['big'], dP, 0, db, 0)
            return torch.cat((dP, db))

    def want(self):
        """The float64 reference as fp32 (after the round-trip check), in the layout `result` returns."""
        from tests.gpu_util import pack
        r = X.reference64(self.o, self.case.op)
        if self.case.op == 2:
            dW = pack(X.to_fp32_exact(r[0]))
            return dW if self.case.klass == 'bf16' else torch.cat((dW, X.to_fp32_exact(r[1])))
        w = B.to_pixels(X.to_fp32_exact(r))
        return w.bfloat16().float() if self.bf[self.out[0]] else w        # (on exact sums round-to-nearest-even is unique)

    def run_compact(self):
        c = {role: self.compact(role) for role, _, _ in self.ins}
        if self.out:
            c[self.out[0]] = self.compact(self.out[0], fill=False)
        flat = self.launch({k: v.v for k, v in c.items()})
        torch.cuda.synchronize()
        return flat if self.out is None else c[self.out[0]].pixels().to(torch.float32, copy=True)

    def run_giant(self, arena, role, tier):
        """The op with `role` giant at `tier`; returns (result, ld, extent, non-NaN found, expected)."""
        _, P, C = next(r for r in self.ins + ([self.out] if self.out else []) if r[0] == role)
        bf = self.bf[role]
        elem = 2 if bf else 4
        ld = B.choose_ld(tier, P, C, elem)
        nbytes = arena.region(P, ld, bf)
        arena.fill(nbytes)
        is_out = self.out is not None and role == self.out[0]
        if not is_out:
            arena.pixels(P, ld, C, bf).copy_(B.to_pixels(self.x[role]))
        views = {role: arena.view(*self.shape[role], ld, bf)}
        c = {}
        for r, _, _ in self.ins + ([self.out] if self.out else []):
            if r != role:
                c[r] = self.compact(r, fill=self.out is None or r != self.out[0])
                views[r] = c[r].v
        err = None
        try:
            flat = self.launch(views)
        except RuntimeError as e:
            err, flat = str(e), getattr(self, 'dP', None)
        torch.cuda.synchronize()
        res = flat if self.out is None else (arena.pixels(P, ld, C, bf) if is_out else c[self.out[0]].pixels()).to(torch.float32, copy=True)
        return res, ld, B.extent(P, ld, C, elem), arena.count(nbytes, bf), (0 if is_out and err else P * C), err


def _diff(got, want):
    bad = ~(got == want)
    return f'{int(bad.sum())} of {got.numel()} differ (NaN: {int(got.isnan().sum())})'


def _run_conv_case(case, tiers):
    arena = _arena(tiers)
    t0 = time.time()
    cv = _Conv(case)
    sym, split = cv.cop.describe(case.op)
    assert sym == case.sym and (case.klass == 'wino1' or B.family_of(sym) == case.family), (case, sym)
    exact = case.klass == 'exact'
    if exact:
        X.budget_for(cv.cpu, case.op, sym)                     # the planned kernel's class ...
        X.budget_for(cv.cpu, case.op, B.GENERIC[case.op])      # ... and the 'gemm' class of the fallbacks beyond the limit
    print(f'{case.family} op {case.op}: {sym} split {split} on {case.geom} algo {case.algo:#x}, tiers {"".join(tiers)}')
    compact = cv.run_compact()
    assert not compact.isnan().any(), f'{case}: the compact call left NaN'
    fails = []
    want = cv.want() if exact else None
    if exact and not torch.equal(compact, want):
        fails.append(f'{case} compact views: not the float64 result: {_diff(compact, want)}')
    for role in [r[0] for r in cv.ins] + ([cv.out[0]] if cv.out else []):
        for tier in tiers:
            got, ld, ext, found, entitled, err = cv.run_giant(arena, role, tier)
            assert err is None, f'{case} giant {role} tier {tier}: {err}'
            print(_line(f'giant {role}', tier, ld, ext, found, entitled))
            tag = f'{case} giant {role} tier {tier} (ld {ld})'
            if found != entitled:
                fails.append(f'{tag}: {found} non-NaN elements in the arena, entitled {entitled}')
            if exact and not torch.equal(got, want):
                fails.append(f'{tag}: not the float64 result: {_diff(got, want)}')
            # tier B is the same kernel (per-element arithmetic does not depend on ld); the stride-1 Winograd paths have no byte limit
            # in the planner, so the same holds for them in every tier
            if (tier == 'B' or case.klass == 'wino1') and not torch.equal(got, compact):
                fails.append(f'{tag}: bits differ from the compact call: {_diff(got, compact)}')
    print(f'  wall {time.time() - t0:.2f} s')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('case', B.exact_cases(), ids=lambda c: c.id)
def test_conv_exact_class(case, group):
    """Every dyadic family: each input giant in turn, then the output, in every tier -- the float64 convolution bit for bit whichever
    kernel the view lands on, tier B bit-identical to the compact call, nothing written outside the output."""
    _run_conv_case(case, GROUPS[group])


@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('case', B.wino1_cases(), ids=lambda c: c.id)
def test_conv_stride1_winograd(case, group):
    """The stride-1 Winograd paths (normal operands; not exact): bit-identical to the compact call in every tier."""
    _run_conv_case(case, GROUPS[group])


@pytest.mark.parametrize('group', list(GROUPS))
def test_bwd_big_on_giant_views(group):
    """pg_conv4x4_bwd_big (weight and data gradient in one call, the transformed dy shared where both run the polyphase path): each of
    its three views giant in turn; dW and the data gradient exact in every tier, tier B bit-identical to compact."""
    from tests.gpu_util import pack
    from tests.test_exact_gpu import _bwd_big_case
    arena = _arena(GROUPS[group])
    t0 = time.time()
    fails = []
    for form in ('s3', 'fp32'):
        geom, algo = _bwd_big_case(form)
        case = B.ConvCase('bwd_big', 0, geom, algo, None, None)
        cv = _Conv(case)
        N, Hb, Wb, Ca, Cb, s = geom
        syms = [cv.cop.describe(i)[0] for i in (0, 2)]
        assert B.family_of(syms[1]) == ('polyphase wgrad s3' if form == 's3' else 'polyphase wgrad fp32'), syms
        for i, sym in zip((0, 2), syms):
            X.budget_for(cv.cpu, i, sym)
            X.budget_for(cv.cpu, i, B.GENERIC[i])
        r2, r0 = X.reference64(cv.o, 2), X.reference64(cv.o, 0, bias=False)
        want = (pack(X.to_fp32_exact(r2[0])), B.to_pixels(X.to_fp32_exact(r0)))
        print(f'bwd_big ({form}): {syms} on {geom} algo {algo:#x}')

        def call(arena, role, tier):
            views, c, info = {}, {}, None
            for r, shape in (('small', cv.shape['small']), ('big', cv.shape['big']), ('dsmall', cv.shape['small'])):
                if r == role:
                    P, C = shape[0] * shape[1] * shape[2], shape[3]
                    ld = B.choose_ld(tier, P, C, 4)
                    nbytes = arena.region(P, ld, False)
                    arena.fill(nbytes)
                    if r != 'dsmall':
                        arena.pixels(P, ld, C).copy_(B.to_pixels(cv.x[r]))
                    views[r], info = arena.view(*shape, ld), (P, C, ld, nbytes)
                else:
                    c[r] = _Compact(*shape, cv.x[r] if r != 'dsmall' else None)
                    views[r] = c[r].v
            dP = _nan(16 * Ca * Cb)
            cv.cop.bwd_big(views['small'], views['big'], cv.pk, dP, 0, views['dsmall'])
            torch.cuda.synchronize()
            ds = (arena.pixels(info[0], info[2], info[1]) if role == 'dsmall' else c['dsmall'].pixels()).clone()
            return (dP, ds), info

        compact, _ = call(None, None, None)
        for k, what in enumerate(('dW', 'data gradient')):
            if not torch.equal(compact[k], want[k]):
                fails.append(f'bwd_big {form} compact {what}: {_diff(compact[k], want[k])}')
        for role in ('small', 'big', 'dsmall'):
            for tier in GROUPS[group]:
                got, (P, C, ld, nbytes) = call(arena, role, tier)
                found = arena.count(nbytes)
                print(_line(f'giant {role}', tier, ld, B.extent(P, ld, C, 4), found, P * C))
                if found != P * C:
                    fails.append(f'bwd_big {form} giant {role} tier {tier}: {found} non-NaN elements in the arena, entitled {P * C}')
                for k, what in enumerate(('dW', 'data gradient')):
                    if not torch.equal(got[k], want[k]):
                        fails.append(f'bwd_big {form} giant {role} tier {tier} {what}: {_diff(got[k], want[k])}')
                    if tier == 'B' and not torch.equal(got[k], compact[k]):
                        fails.append(f'bwd_big {form} giant {role} tier B {what}: bits differ from compact')
    print(f'  wall {time.time() - t0:.2f} s')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('family,op', B.HANDOVER,ids=lambda v: str(v).replace(' ', '_'))
def test_handovers_decline_beyond_the_limit(family, op, group):
    """ConvOp.fits: for a giant view of tiers A, S and W the engine plans no partial sums, no weight cache and no epilogue multiplier
    (on compact views it plans the first two: the precondition that makes declining mean something).  A direct call with `part` on
    such a view returns PG_EINVAL with nothing written, or PG_OK with the output and the partial sums exact (the polyphase path has
    no limit and may run)."""
    from patchgan_amd import engine as E
    arena = _arena(GROUPS[group])
    tiers = [t for t in GROUPS[group] if t != 'B']
    t0 = time.time()
    case = B.handover_case(family, op)
    cv = _Conv(case)
    cop, o = cv.cop, cv.o
    rin, rout = cv.ins[0][0], cv.out[0]
    N, Ho, Wo, Co = cv.shape[rout]
    cin, cout = cv.compact(rin), cv.compact(rout, fill=False)
    chunks = cop.stats_chunks(op, cin.v, cout.v)
    assert chunks > 0, f'{case}: no partial sums on compact views'
    if family.startswith('polyphase'):
        assert E._ucache(E.UCache(), ('t', 0), op, cop, torch.device(DEV), cin.v, cout.v, 0)[0] is not None
    if op == 1 and family.startswith('polyphase'):
        assert cop.mul_ok(cin.v, cout.v, cv.compact(rout).v)
    want = B.to_pixels(X.to_fp32_exact(X.reference64(o, op, bias=False)))
    w64 = B.from_pixels(want, N, Ho, Wo).double()
    print(f'{case}: {chunks} partial-sum chunks per sample on compact views')
    fails = []
    for role in (rin, rout):
        _, P, C = next(r for r in cv.ins + [cv.out] if r[0] == role)
        for tier in tiers:
            ld = B.choose_ld(tier, P, C, 4)
            nbytes = arena.region(P, ld, False)
            arena.fill(nbytes)
            gv = arena.view(*cv.shape[role], ld)
            if role == rin:
                arena.pixels(P, ld, C).copy_(B.to_pixels(cv.x[role]))
                vin, other = gv, cv.compact(rout, fill=False)
                vout = other.v
            else:
                other = cv.compact(rin)
                vin, vout = other.v, gv
            tag = f'{case} giant {role} tier {tier}'
            assert cop.stats_chunks(op, vin, vout) == 0, tag
            assert E._ucache(E.UCache(), ('t', 0), op, cop, torch.device(DEV), vin, vout, 0) == (None, False), tag
            if op == 1:
                assert not cop.mul_ok(vin, vout, cv.compact(rout).v), tag
            part = _nan(N * chunks * Co * 2, torch.float64)
            call = cop.big2small if op == 0 else cop.small2big
            views = (vin, cv.pk, 0, None, 0, vout)
            try:
                call(*views, part=part)
                rc = 'PG_OK'
            except RuntimeError as e:
                assert 'PG_EINVAL' in str(e), e
                rc = 'PG_EINVAL'
            torch.cuda.synchronize()
            found = arena.count(nbytes)
            entitled = P * C if (role == rin or rc == 'PG_OK') else 0
            print(_line(f'part, giant {role}: {rc}', tier, ld, B.extent(P, ld, C, 4), found, entitled))
            if found != entitled:
                fails.append(f'{tag} ({rc}): {found} non-NaN elements in the arena, entitled {entitled}')
            got = (arena.pixels(P, ld, C) if role == rout else other.pixels()).clone()
            if rc == 'PG_EINVAL':
                if not (bool(part.isnan().all()) and (role == rout or bool(got.isnan().all()))):
                    fails.append(f'{tag}: PG_EINVAL, but something was written')
            else:
                sums = part.view(N, chunks, Co, 2).sum(1)
                if not torch.equal(got, want):
                    fails.append(f'{tag}: PG_OK, output: {_diff(got, want)}')
                if not (torch.equal(sums[..., 0], w64.sum((2, 3))) and torch.equal(sums[..., 1], (w64 * w64).sum((2, 3)))):
                    fails.append(f'{tag}: PG_OK, but the partial sums are not exact')
    print(f'  wall {time.time() - t0:.2f} s')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('family', ['polyphase s3', 'ca1'])
def test_epilogue_multiplier_giant_below_the_limit(family):
    """pg_conv_extras.mul_t (big = conv * f'(t)) with t giant in tier B: bit-identical to the call with t compact, t untouched."""
    t0 = time.time()
    case = B.exact_case(family, 1)
    cv = _Conv(case)
    arena = _arena(())
    N, Hb, Wb, Cb = cv.shape['big']
    P = N * Hb * Wb
    t = (cv.o.big - 0.5) * 0.25          # both signs, no zero: the LeakyReLU derivative takes both of its values
    small = cv.compact('small')

    def call(tv):
        out = cv.compact('big', fill=False)
        cv.cop.small2big(small.v, cv.pk, 0, cv.o.bias_b, 0, out.v, L.ACT_NONE, mul=(tv, L.ACT_LEAKY))
        torch.cuda.synchronize()
        return out.pixels().clone()
    tc = _Compact(N, Hb, Wb, Cb, t)
    assert cv.cop.mul_ok(small.v, cv.compact('big', fill=False).v, tc.v), case
    compact = call(tc.v)
    plain = cv.run_compact()
    assert not compact.isnan().any() and not torch.equal(compact, plain), 'the multiplier did nothing'
    ld = B.choose_ld('B', P, Cb, 4)
    nbytes = arena.region(P, ld, False)
    arena.fill(nbytes)
    arena.pixels(P, ld, Cb).copy_(B.to_pixels(t))
    got = call(arena.view(N, Hb, Wb, Cb, ld))
    found = arena.count(nbytes)
    print(f'{case}: mul_t')
    print(_line('giant mul_t', 'B', ld, B.extent(P, ld, Cb, 4), found, P * Cb))
    print(f'  wall {time.time() - t0:.2f} s')
    assert found == P * Cb and torch.equal(arena.pixels(P, ld, Cb), B.to_pixels(t))
    assert torch.equal(got, compact), _diff(got, compact)


@pytest.mark.parametrize('case', B.bf16_cases(), ids=lambda c: c.id)
def test_conv_bf16_tensors(case):
    """bf16 tensors (PG_IO_*): tier B runs and gives the nearest-even rounding of the exact sum; tiers A and S have no kernel --
    PG_EINVAL with nothing written, neither in the arena nor in the compact output."""
    arena = _arena(())
    t0 = time.time()
    cv = _Conv(case)
    sym, split = cv.cop.describe(case.op, case.io)
    assert sym == case.sym, (case, sym)
    X.budget_for(cv.cpu, case.op, sym)
    print(f'{case.family} op {case.op}: {sym} split {split} on {case.geom} algo {case.algo:#x} io {case.io:#x}, tiers BAS')
    want, compact = cv.want(), cv.run_compact()
    fails = []
    if not torch.equal(compact, want):
        fails.append(f'{case} compact views: {_diff(compact, want)}')
    for role in [r[0] for r in cv.ins + ([cv.out] if cv.out else []) if cv.bf[r[0]]]:
        is_out = cv.out is not None and role == cv.out[0]
        for tier in ('B', 'A', 'S'):
            got, ld, ext, found, entitled, err = cv.run_giant(arena, role, tier)
            print(_line(f'giant {role}: {"PG_OK" if err is None else err}', tier, ld, ext, found, entitled))
            tag = f'{case} giant {role} tier {tier} (ld {ld})'
            if found != entitled:
                fails.append(f'{tag}: {found} non-NaN elements in the arena, entitled {entitled}')
            if tier == 'B':
                if err is not None:
                    fails.append(f'{tag}: {err}')
                elif not (torch.equal(got, want) and torch.equal(got, compact)):
                    fails.append(f'{tag}: {_diff(got, want)}')
            elif err is None or 'PG_EINVAL' not in err:
                fails.append(f'{tag}: a bf16 tensor beyond the limit has no kernel, but the call returned {err or "PG_OK"}')
            elif not is_out and not bool(got.isnan().all()):
                fails.append(f'{tag}: PG_EINVAL, but the compact output was written')
    print(f'  wall {time.time() - t0:.2f} s')
    assert not fails, '\n'.join(fails)


# ---- Part 2: norm, activation, BatchNorm, loss, layout, metrics, diffaug and tile kernels ------------------------------------------------
# These kernels have no limit switch: tiers S and W (bf16 views: S), one operand giant at a time, bit-identity with the same call on
# compact views (same alignment: ld a multiple of the vector width, 16-byte-aligned bases) plus the non-NaN count.
class _Op:
    """One entry point: `tensors` = [(key, 'in' | 'out', C, bf16?)] are its [P][C] views (P pixels each, or a (P, C, ...) override
    in `pix`); make() -> state (the inputs' [P][C] data under their keys, anything else the call needs); call(state, a) with
    a[key] = (device address, ld) launches and returns {name: small output tensor}."""

    def __init__(self, name, P, tensors, make, call, pix=None):
        self.name, self.P, self.tensors, self.make, self.call, self.pix = name, P, tensors, make, call, pix or {}
        for key, kind, C, bf in tensors:
            B.part2_view(f'{name} {key}', 1, 1, self.pix.get(key, P), C, 2 if bf else 4)


def _st():
    from patchgan_amd import engine as E
    return E._stream()


def _rnd(seed, P, C, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, C, generator=g) * (hi - lo) + lo).to(DEV)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def _ok(rc, what):
    L.check(rc, what)


def _instnorm_ops():
    lib = L.load()
    ops = []
    for tag, N, HW, C in (('single-workgroup', 2, 96, 8), ('chunked', 2, 576, 8)):
        P = N * HW
        wsb = int(lib.pg_instnorm_affine_workspace_bytes(N, HW, C))

        def make(N=N, HW=HW, C=C, P=P, wsb=wsb):
            s = {'y': _rnd(1, P, C, -2, 2), 'g1': _rnd(2, P, C), 'g2': _rnd(3, P, C), 'gamma': _rnd(4, 1, C, 0.5, 1.5).view(-1).contiguous(),
                 'beta': _rnd(5, 1, C).view(-1).contiguous(), 'ws': _ws(wsb), 'stats': _nan(N * C * 2)}
            yc = _Compact(1, 1, P, C, None)
            yc.pixels().copy_(s['y'])
            out = _Compact(1, 1, P, C, None)
            _ok(lib.pg_instnorm_act_fwd(yc.v.ptr(), yc.ld, out.v.ptr(), out.ld, s['stats'].data_ptr(), N, HW, C, L.ACT_LEAKY, 1e-5, 0.0, 0,
                                        s['ws'].data_ptr(), wsb, _st()), 'pg_instnorm_act_fwd')
            y64 = s['y'].double().view(N, 3, HW // 3, C)
            s['part'] = torch.stack((y64.sum(2), (y64 * y64).sum(2)), -1).contiguous()      # [N][3 chunks][C][2]
            for k in ('y', 'g1', 'g2'):
                s[k + '_bf'] = s[k].bfloat16()
            return s
        for dt, sfx in ((0, ''), (1, ' bf16')):
            bf = bool(dt)
            k = (lambda key, bf=bf: key + '_bf' if bf else key)

            def fwd(s, a, N=N, HW=HW, C=C, wsb=wsb, bf=bf):
                st = _nan(N * C * 2)
                _ok(lib.pg_instnorm_act_fwd_t(a['y'][0], a['y'][1], a['out'][0], a['out'][1], st.data_ptr(), N, HW, C, L.ACT_LEAKY, 1e-5, 0.25, 77,
                                              s['ws'].data_ptr(), wsb, _st(), 3 if bf else 0), 'pg_instnorm_act_fwd_t')
                return {'stats': st}

            def bwd(s, a, N=N, HW=HW, C=C, wsb=wsb, bf=bf):
                _ok(lib.pg_instnorm_act_bwd_t(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['y'][0], a['y'][1], s['stats'].data_ptr(),
                                              a['dy'][0], a['dy'][1], N, HW, C, L.ACT_LEAKY, 0.25, 77, s['ws'].data_ptr(), wsb, _st(),
                                              15 if bf else 0), 'pg_instnorm_act_bwd_t')
                return {}
            ops.append(_Op(f'instnorm_act_fwd{"_t" if bf else ""} {tag}{sfx}', P, [('y', 'in', C, bf), ('out', 'out', C, bf)], make, fwd))
            ops.append(_Op(f'instnorm_act_bwd{"_t" if bf else ""} {tag}{sfx}', P,
                           [('g1', 'in', C, bf), ('g2', 'in', C, bf), ('y', 'in', C, bf), ('dy', 'out', C, bf)], make, bwd))

        def plain_fwd(s, a, N=N, HW=HW, C=C, wsb=wsb):
            st = _nan(N * C * 2)
            _ok(lib.pg_instnorm_act_fwd(a['y'][0], a['y'][1], a['out'][0], a['out'][1], st.data_ptr(), N, HW, C, L.ACT_RELU, 1e-5, 0.0, 0,
                                        s['ws'].data_ptr(), wsb, _st()), 'pg_instnorm_act_fwd')
            return {'stats': st}

        def plain_bwd(s, a, N=N, HW=HW, C=C, wsb=wsb):
            _ok(lib.pg_instnorm_act_bwd(a['g1'][0], a['g1'][1], None, 0, a['y'][0], a['y'][1], s['stats'].data_ptr(), a['dy'][0], a['dy'][1],
                                        N, HW, C, L.ACT_RELU, 0.0, 0, s['ws'].data_ptr(), wsb, _st()), 'pg_instnorm_act_bwd')
            return {}

        def parts(s, a, N=N, HW=HW, C=C):
            st = _nan(N * C * 2)
            _ok(lib.pg_instnorm_act_fwd_parts(a['y'][0], a['y'][1], a['out'][0], a['out'][1], st.data_ptr(), s['part'].data_ptr(), 3, N, HW, C,
                                              L.ACT_LEAKY, 1e-5, 0.0, 0, _st()), 'pg_instnorm_act_fwd_parts')
            return {'stats': st}

        def aff_fwd(s, a, N=N, HW=HW, C=C, wsb=wsb):
            st = _nan(N * C * 2)
            _ok(lib.pg_instnorm_affine_act_fwd_t(a['y'][0], a['y'][1], a['out'][0], a['out'][1], s['gamma'].data_ptr(), s['beta'].data_ptr(),
                                                 st.data_ptr(), N, HW, C, L.ACT_LEAKY, 1e-5, 0.0, 0, s['ws'].data_ptr(), wsb, _st(), 0),
                'pg_instnorm_affine_act_fwd_t')
            return {'stats': st}

        def aff_bwd(s, a, N=N, HW=HW, C=C, wsb=wsb):
            dg, db = _nan(C), _nan(C)
            _ok(lib.pg_instnorm_affine_act_bwd_t(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['y'][0], a['y'][1], s['gamma'].data_ptr(),
                                                 s['beta'].data_ptr(), s['stats'].data_ptr(), a['dy'][0], a['dy'][1], dg.data_ptr(), db.data_ptr(),
                                                 N, HW, C, L.ACT_LEAKY, 0.0, 0, s['ws'].data_ptr(), wsb, _st(), 0), 'pg_instnorm_affine_act_bwd_t')
            return {'dgamma': dg, 'dbeta': db}
        io2 = [('y', 'in', C, False), ('out', 'out', C, False)]
        io4 = [('g1', 'in', C, False), ('g2', 'in', C, False), ('y', 'in', C, False), ('dy', 'out', C, False)]
        ops += [_Op(f'instnorm_act_fwd plain {tag}', P, io2, make, plain_fwd),
                _Op(f'instnorm_act_bwd plain no g2 {tag}', P, [io4[0], io4[2], io4[3]], make, plain_bwd),
                _Op(f'instnorm_act_fwd_parts {tag}', P, io2, make, parts),
                _Op(f'instnorm_affine_act_fwd {tag}', P, io2, make, aff_fwd),
                _Op(f'instnorm_affine_act_bwd {tag}', P, io4, make, aff_bwd)]
    return ops


def _act_ops():
    lib = L.load()
    P, C, Cs = 1500, 8, 5

    def make():
        s = {'y': _rnd(11, P, C, -2, 2), 'g1': _rnd(12, P, C), 'g2': _rnd(13, P, C), 'ys': _rnd(14, P, Cs, -3, 3), 'g1s': _rnd(15, P, Cs), 'g2s': _rnd(16, P, Cs)}
        s['a'] = torch.tanh(s['y'])
        s['outs'] = torch.softmax(s['ys'], 1)
        return s

    def act_fwd(s, a):
        _ok(lib.pg_act_fwd(a['y'][0], a['y'][1], a['out'][0], a['out'][1], P, C, L.ACT_TANH, 0.25, 5, _st()), 'pg_act_fwd')
        return {}

    def act_bwd(s, a):
        _ok(lib.pg_act_bwd(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['a'][0], a['a'][1], a['dy'][0], a['dy'][1], P, C, L.ACT_TANH, 0.0, 0,
                           _st()), 'pg_act_bwd')
        return {}

    def sm_fwd(s, a):
        _ok(lib.pg_softmax_fwd(a['ys'][0], a['ys'][1], a['out'][0], a['out'][1], P, Cs, _st()), 'pg_softmax_fwd')
        return {}

    def sm_bwd(s, a):
        _ok(lib.pg_softmax_bwd(a['g1s'][0], a['g1s'][1], a['g2s'][0], a['g2s'][1], a['outs'][0], a['outs'][1], a['dy'][0], a['dy'][1], P, Cs,
                               _st()), 'pg_softmax_bwd')
        return {}
    return [_Op('act_fwd', P, [('y', 'in', C, False), ('out', 'out', C, False)], make, act_fwd),
            _Op('act_bwd', P, [('g1', 'in', C, False), ('g2', 'in', C, False), ('a', 'in', C, False), ('dy', 'out', C, False)], make, act_bwd),
            _Op('softmax_fwd', P, [('ys', 'in', Cs, False), ('out', 'out', Cs, False)], make, sm_fwd),
            _Op('softmax_bwd', P, [('g1s', 'in', Cs, False), ('g2s', 'in', Cs, False), ('outs', 'in', Cs, False), ('dy', 'out', Cs, False)], make, sm_bwd)]


def _batchnorm_ops():
    lib = L.load()
    ops = []
    for nseg, HW in ((1, 96), (2, 96), (1, 576), (2, 576)):
        N, C = 2, 8
        P = N * HW
        wsb = int(lib.pg_batchnorm_workspace_bytes(N, HW, C, nseg))
        count = float(N // nseg * HW)
        tag = f'nseg {nseg} HW {HW}'

        def make(N=N, HW=HW, C=C, P=P, wsb=wsb, nseg=nseg):
            s = {'y': _rnd(21, P, C, -2, 2), 'g1': _rnd(22, P, C), 'g2': _rnd(23, P, C), 'w': _rnd(24, 1, C, 0.5, 1.5).view(-1).contiguous(),
                 'b': _rnd(25, 1, C).view(-1).contiguous(), 'ws': _ws(wsb), 'coef': _nan(nseg * C * 4), 'mom': _nan(nseg * C * 2, torch.float64)}
            yc, g1, g2 = (_Compact(1, 1, P, C, None) for _ in range(3))
            for c, k in ((yc, 'y'), (g1, 'g1'), (g2, 'g2')):
                c.pixels().copy_(s[k])
            _ok(lib.pg_batchnorm_stats(yc.v.ptr(), yc.ld, None, 0, s['w'].data_ptr(), s['b'].data_ptr(), s['coef'].data_ptr(), None, N, HW, C, nseg,
                                       1e-5, s['ws'].data_ptr(), wsb, _st()), 'pg_batchnorm_stats')
            _ok(lib.pg_batchnorm_moments_bwd(g1.v.ptr(), g1.ld, g2.v.ptr(), g2.ld, yc.v.ptr(), yc.ld, s['coef'].data_ptr(), s['mom'].data_ptr(),
                                             None, None, N, HW, C, nseg, L.ACT_LEAKY, 0.0, 0, s['ws'].data_ptr(), wsb, _st()), 'pg_batchnorm_moments_bwd')
            torch.cuda.synchronize()
            return s

        def fwd(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg):
            coef, bstat = _nan(nseg * C * 4), _nan(nseg * C * 2, torch.float64)
            _ok(lib.pg_batchnorm_act_fwd(a['y'][0], a['y'][1], a['out'][0], a['out'][1], s['w'].data_ptr(), s['b'].data_ptr(), coef.data_ptr(),
                                         bstat.data_ptr(), N, HW, C, nseg, L.ACT_LEAKY, 1e-5, 0.25, 9, s['ws'].data_ptr(), wsb, _st()), 'pg_batchnorm_act_fwd')
            return {'coef': coef, 'bstat': bstat}

        def stats(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg):
            coef, bstat = _nan(nseg * C * 4), _nan(nseg * C * 2, torch.float64)
            _ok(lib.pg_batchnorm_stats(a['y'][0], a['y'][1], None, 0, s['w'].data_ptr(), s['b'].data_ptr(), coef.data_ptr(), bstat.data_ptr(), N, HW, C,
                                       nseg, 1e-5, s['ws'].data_ptr(), wsb, _st()), 'pg_batchnorm_stats')
            return {'coef': coef, 'bstat': bstat}

        def apply(s, a, N=N, HW=HW, C=C, nseg=nseg):
            _ok(lib.pg_batchnorm_act_apply(a['y'][0], a['y'][1], a['out'][0], a['out'][1], s['coef'].data_ptr(), N, HW, C, nseg, L.ACT_LEAKY, 0.25, 9,
                                           _st()), 'pg_batchnorm_act_apply')
            return {}

        def bwd(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg):
            dw, db = _nan(C), _nan(C)
            _ok(lib.pg_batchnorm_act_bwd(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['y'][0], a['y'][1], s['coef'].data_ptr(), a['dy'][0],
                                         a['dy'][1], dw.data_ptr(), db.data_ptr(), N, HW, C, nseg, 1, L.ACT_LEAKY, 0.0, 0, s['ws'].data_ptr(), wsb,
                                         _st()), 'pg_batchnorm_act_bwd')
            return {'dweight': dw, 'dbias': db}

        def mom_fwd(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg):
            mom = _nan(nseg * C * 2, torch.float64)
            _ok(lib.pg_batchnorm_moments_fwd(a['y'][0], a['y'][1], None, 0, mom.data_ptr(), N, HW, C, nseg, s['ws'].data_ptr(), wsb, _st()),
                'pg_batchnorm_moments_fwd')
            return {'mom': mom}

        def mom_bwd(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg):
            mom, dw, db = _nan(nseg * C * 2, torch.float64), _nan(C), _nan(C)
            _ok(lib.pg_batchnorm_moments_bwd(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['y'][0], a['y'][1], s['coef'].data_ptr(), mom.data_ptr(),
                                             dw.data_ptr(), db.data_ptr(), N, HW, C, nseg, L.ACT_LEAKY, 0.0, 0, s['ws'].data_ptr(), wsb, _st()),
                'pg_batchnorm_moments_bwd')
            return {'mom': mom, 'dweight': dw, 'dbias': db}

        def bwd_apply(s, a, N=N, HW=HW, C=C, wsb=wsb, nseg=nseg, count=count):
            _ok(lib.pg_batchnorm_bwd_apply(a['g1'][0], a['g1'][1], a['g2'][0], a['g2'][1], a['y'][0], a['y'][1], s['coef'].data_ptr(), s['mom'].data_ptr(),
                                           count, a['dy'][0], a['dy'][1], N, HW, C, nseg, L.ACT_LEAKY, 0.0, 0, s['ws'].data_ptr(), wsb, _st()),
                'pg_batchnorm_bwd_apply')
            return {}
        y, out = ('y', 'in', C, False), ('out', 'out', C, False)
        g3 = [('g1', 'in', C, False), ('g2', 'in', C, False), y]
        ops += [_Op(f'batchnorm_act_fwd {tag}', P, [y, out], make, fwd), _Op(f'batchnorm_stats {tag}', P, [y], make, stats),
                _Op(f'batchnorm_act_apply {tag}', P, [y, out], make, apply), _Op(f'batchnorm_act_bwd {tag}', P, g3 + [('dy', 'out', C, False)], make, bwd),
                _Op(f'batchnorm_moments_fwd {tag}', P, [y], make, mom_fwd), _Op(f'batchnorm_moments_bwd {tag}', P, g3, make, mom_bwd),
                _Op(f'batchnorm_bwd_apply {tag}', P, g3 + [('dy', 'out', C, False)], make, bwd_apply)]
    return ops


def _loss_ops():
    lib = L.load()
    N, HW, C = 2, 576, 3
    P = N * HW
    nd = int(lib.pg_loss_reduce_doubles(N, HW, C))

    def make():
        s = {'p': _rnd(31, P, C, 0.05, 0.95), 'y': (_rnd(32, P, C, 0, 1) > 0.6).float(), 'coef': _rnd(33, 1, N * C * 2).view(-1).contiguous()}
        pc, yc = _Compact(1, 1, P, C, None), _Compact(1, 1, P, C, None)
        pc.pixels().copy_(s['p'])
        yc.pixels().copy_(s['y'])
        s['Spart'] = _nan(nd, torch.float64)
        s['nsplit'] = int(lib.pg_loss_reduce_parts(pc.v.ptr(), pc.ld, yc.v.ptr(), yc.ld, 0.0, N, HW, C, s['Spart'].data_ptr(), _st()))
        assert s['nsplit'] >= 1
        torch.cuda.synchronize()
        return s

    def reduce(s, a):
        S = _nan(nd, torch.float64)
        _ok(lib.pg_loss_reduce(a['p'][0], a['p'][1], a['y'][0], a['y'][1], 0.0, N, HW, C, S.data_ptr(), _st()), 'pg_loss_reduce')
        return {'S': S[:N * C * 5]}

    def reduce_parts(s, a):
        S = _nan(nd, torch.float64)
        n = int(lib.pg_loss_reduce_parts(a['p'][0], a['p'][1], a['y'][0], a['y'][1], 0.0, N, HW, C, S.data_ptr(), _st()))
        assert n == s['nsplit'], n
        return {'S': S[:n * N * C * 5]}

    def grad(s, a):
        _ok(lib.pg_loss_grad(a['p'][0], a['p'][1], a['y'][0], a['y'][1], 0.0, s['coef'].data_ptr(), a['g'][0], a['g'][1], N, HW, C, 1, _st()), 'pg_loss_grad')
        return {}

    def value_grad(s, a):
        S_out, loss = _nan(N * C * 5, torch.float64), _nan(1)
        _ok(lib.pg_loss_value_grad(s['Spart'].data_ptr(), s['nsplit'], S_out.data_ptr(), None, L.LOSS_WBCE, N, C, HW, N, 1.0, 0.75, 0.75, a['p'][0], a['p'][1],
                                   a['y'][0], a['y'][1], 0.0, a['g'][0], a['g'][1], loss.data_ptr(), _st()), 'pg_loss_value_grad')
        return {'S_out': S_out, 'loss': loss}
    p, y, g = ('p', 'in', C, False), ('y', 'in', C, False), ('g', 'out', C, False)
    ops = [_Op('loss_reduce', P, [p, y], make, reduce), _Op('loss_reduce_parts', P, [p, y], make, reduce_parts), _Op('loss_grad', P, [p, y, g], make, grad),
           _Op('loss_value_grad', P, [p, y, g], make, value_grad)]
    for tag, n in (('one launch', 2 * 30 * 30), ('slabs', 2 * 96 * 96)):
        def gmake(n=n):
            return {'d': _rnd(41, n, 1, -3, 3)}

        def gan(s, a, n=n):
            value = _nan(1)
            term = L.GanTerm(a['d'][0], a['g'][0], value.data_ptr(), 0.5 / n, n, a['d'][1], a['g'][1], L.GAN_BCE_LOGITS, 1.0)
            arr = (L.GanTerm * 1)(term)
            wsb = int(lib.pg_gan_loss_workspace_bytes(1, arr))
            assert (wsb > 0) == (n > int(lib.pg_gan_loss_single_max())), (n, wsb)
            ws = _ws(wsb)
            _ok(lib.pg_gan_loss(1, arr, ws.data_ptr() if wsb else None, wsb, _st()), 'pg_gan_loss')
            return {'value': value}
        ops.append(_Op(f'gan_loss {tag}', n, [('d', 'in', 1, False), ('g', 'out', 1, False)], gmake, gan))
    return ops


def _metrics_ops():
    lib = L.load()
    N, HW, C, bins = 2, 600, 3, 16
    P = N * HW

    def make():
        y = torch.nn.functional.one_hot((_rnd(52, P, 1, 0, 3.999).long().view(-1)) % 4, 4)[:, :C].float()       # (class 3: no listed label)
        return {'p': _rnd(51, P, C, 0, 1), 'y': y.contiguous()}

    def confusion(s, a):
        counts = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
        _ok(lib.pg_seg_confusion(a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, 0.5, counts.data_ptr(), _st()), 'pg_seg_confusion')
        return {'counts': counts}

    def hist(s, a):
        h = torch.zeros(C * 2 * bins + 1, dtype=torch.int64, device=DEV)
        _ok(lib.pg_seg_hist(a['p'][0], a['p'][1], a['y'][0], a['y'][1], N, HW, C, bins, h.data_ptr(), _st()), 'pg_seg_hist')
        return {'hist': h}
    p, y = ('p', 'in', C, False), ('y', 'in', C, False)
    return [_Op('seg_confusion', P, [p, y], make, confusion), _Op('seg_hist', P, [p, y], make, hist)]


def _layout_ops():
    lib = L.load()
    N, C, H, W = 2, 3, 20, 25
    P = N * H * W

    def make():
        g = torch.Generator().manual_seed(61)
        x = _rnd(61, P, C)
        return {'x': x, 'nchw': B.from_pixels(x, N, H, W), 'u8': torch.randint(0, 256, (P, C), generator=g, dtype=torch.uint8).to(DEV),
                'lab': torch.randint(0, 256, (P,), generator=g, dtype=torch.uint8).to(DEV)}

    def to_nhwc(s, a):
        _ok(lib.pg_nchw_to_nhwc(s['nchw'].data_ptr(), a['dst'][0], a['dst'][1], N, C, H, W, _st()), 'pg_nchw_to_nhwc')
        return {}

    def to_nchw(s, a):
        out = _nan(P * C)
        _ok(lib.pg_nhwc_to_nchw(a['x'][0], a['x'][1], out.data_ptr(), N, C, H, W, _st()), 'pg_nhwc_to_nchw')
        return {'nchw': out}

    def copy(s, a):
        _ok(lib.pg_copy_channels(a['x'][0], a['x'][1], a['dst'][0], a['dst'][1], P, C, _st()), 'pg_copy_channels')
        return {}

    def u8(s, a):
        _ok(lib.pg_u8_to_f32(s['u8'].data_ptr(), a['dst'][0], a['dst'][1], P, C, 255.0, _st()), 'pg_u8_to_f32')
        return {}

    def onehot(s, a):
        labels = (ctypes.c_int * C)(0, 1, 7)
        _ok(lib.pg_labels_to_onehot(s['lab'].data_ptr(), a['dst'][0], a['dst'][1], P, labels, C, 1, _st()), 'pg_labels_to_onehot')
        return {}

    def pad8(s, a):
        out = torch.full((P * 8,), NAN, dtype=torch.bfloat16, device=DEV)
        _ok(lib.pg_pad8_bf16(a['x'][0], a['x'][1], out.data_ptr(), P, C, _st()), 'pg_pad8_bf16')
        return {'pad8': out}
    x, dst = ('x', 'in', C, False), ('dst', 'out', C, False)
    return [_Op('nchw_to_nhwc', P, [dst], make, to_nhwc), _Op('nhwc_to_nchw', P, [x], make, to_nchw), _Op('copy_channels', P, [x, dst], make, copy),
            _Op('u8_to_f32', P, [dst], make, u8), _Op('labels_to_onehot', P, [dst], make, onehot), _Op('pad8_bf16', P, [x], make, pad8)]


def _diffaug_ops():
    lib = L.load()
    N, H, W, C = 3, 16, 24, 4
    P = N * H * W

    def make():
        params = torch.zeros(N * 8, dtype=torch.int32, device=DEV)
        _ok(lib.pg_diffaug_params(1234, None, 3, 7, 0, N, H, W, params.data_ptr(), _st()), 'pg_diffaug_params')
        return {'x': _rnd(71, P, C), 'params': params}

    def fwd(s, a):
        _ok(lib.pg_diffaug_fwd(a['x'][0], a['x'][1], a['dst'][0], a['dst'][1], s['params'].data_ptr(), N, H, W, C, _st()), 'pg_diffaug_fwd')
        return {}

    def bwd(s, a):
        _ok(lib.pg_diffaug_bwd(a['x'][0], a['x'][1], a['dst'][0], a['dst'][1], s['params'].data_ptr(), N, H, W, C, _st()), 'pg_diffaug_bwd')
        return {}
    io = [('x', 'in', C, False), ('dst', 'out', C, False)]
    return [_Op('diffaug_fwd', P, io, make, fwd), _Op('diffaug_bwd', P, io, make, bwd)]


def _tile_ops():
    lib = L.load()
    C, H, W, size, eff = 3, 40, 36, 16, 8
    T = int(lib.pg_tiles_count(H, size, eff)) * int(lib.pg_tiles_count(W, size, eff))
    ops = []
    for K in (1, 2):
        P = K * T * size * size

        def make(P=P):
            g = torch.Generator().manual_seed(81)
            win = (torch.rand(size, generator=g, dtype=torch.float64) + 0.5).to(DEV)
            return {'image': _rnd(81, C * H * W, 1).view(-1).contiguous(), 'tiles': _rnd(82, P, C, 0, 1), 'win': win}

        def gather(s, a, K=K):
            if K == 1:
                _ok(lib.pg_tiles_gather(s['image'].data_ptr(), C, H, W, size, eff, a['out'][0], a['out'][1], _st()), 'pg_tiles_gather')
            else:
                _ok(lib.pg_tiles_gather_tta(s['image'].data_ptr(), C, H, W, size, eff, K, a['out'][0], a['out'][1], _st()), 'pg_tiles_gather_tta')
            return {}

        def blend(s, a, K=K):
            mask, arg = _nan(C * H * W, torch.float64), torch.full((H * W,), -1, dtype=torch.int64, device=DEV)
            if K == 1:
                _ok(lib.pg_tiles_blend(a['tiles'][0], a['tiles'][1], C, size, eff, H, W, 0.0, mask.data_ptr(), arg.data_ptr(), _st()), 'pg_tiles_blend')
            else:
                _ok(lib.pg_tiles_blend_win(a['tiles'][0], a['tiles'][1], C, size, eff, H, W, K, s['win'].data_ptr(), 0.0, mask.data_ptr(), arg.data_ptr(),
                                           _st()), 'pg_tiles_blend_win')
            return {'mask': mask, 'argmax': arg}
        ops += [_Op('tiles_gather' if K == 1 else 'tiles_gather_tta', P, [('out', 'out', C, False)], make, gather),
                _Op('tiles_blend' if K == 1 else 'tiles_blend_win', P, [('tiles', 'in', C, False)], make, blend)]
    return ops


PART2 = {'instnorm': _instnorm_ops(), 'act_softmax': _act_ops(), 'batchnorm': _batchnorm_ops(), 'loss': _loss_ops(), 'metrics': _metrics_ops(),
         'layout': _layout_ops(), 'diffaug': _diffaug_ops(), 'tiles': _tile_ops()}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def _run_op(op, arena, giant, tier):
    """One call of `op` with the view `giant` (None: all compact) at `tier`; returns ({name: result}, ld, extent, found, entitled)."""
    s = op.state
    a, keep, info = {}, {}, None
    for key, kind, C, bf in op.tensors:
        P = op.pix.get(key, op.P)
        data = s[key + '_bf' if bf else key] if kind == 'in' else None
        if key == giant:
            ld = B.choose_ld(tier, P, C, 2 if bf else 4)
            nbytes = arena.region(P, ld, bf)
            arena.fill(nbytes)
            if data is not None:
                arena.pixels(P, ld, C, bf).copy_(data)
            a[key] = (arena.view(1, 1, P, C, ld, bf).ptr(), ld)
            info = (P, C, bf, ld, nbytes)
        else:
            c = keep[key] = _Compact(1, 1, P, C, None, bf)
            if data is not None:
                c.pixels().copy_(data)
            a[key] = (c.v.ptr(), c.ld)
    res = dict(op.call(s, a))
    torch.cuda.synchronize()
    for key, kind, C, bf in op.tensors:
        if kind == 'out':
            res[key] = (arena.pixels(info[0], info[3], C, bf) if key == giant else keep[key].pixels()).clone()
    if giant is None:
        return res
    P, C, bf, ld, nbytes = info
    return res, ld, B.extent(P, ld, C, 2 if bf else 4), arena.count(nbytes, bf), P * C


@pytest.mark.parametrize('tier', ['S', 'W'])
@pytest.mark.parametrize('group', list(PART2))
def test_part2_kernels(group, tier):
    arena = _arena((tier,))
    t0 = time.time()
    fails = []
    for op in PART2[group]:
        op.state = op.make()
        compact = _run_op(op, arena, None, None)
        assert all(not v.isnan().any() for v in compact.values() if v.is_floating_point()), f'{op.name}: the compact call left NaN'
        print(f'{op.name}: {sorted(compact)}')
        for key, kind, C, bf in op.tensors:
            if bf and tier == 'W':
                continue            # (2^32 bytes of bf16 are 2^31 elements: out of scope)
            got, ld, ext, found, entitled = _run_op(op, arena, key, tier)
            print(_line(f'giant {key}', tier, ld, ext, found, entitled))
            if found != entitled:
                fails.append(f'{op.name} giant {key} tier {tier}: {found} non-NaN elements in the arena, entitled {entitled}')
            for name in compact:
                if not torch.equal(_bits(got[name]), _bits(compact[name])):
                    fails.append(f'{op.name} giant {key} tier {tier}: {name} differs from the compact call in '
                                 f'{int((_bits(got[name]) != _bits(compact[name])).sum())} of {compact[name].numel()} elements')
        del op.state
    print(f'  wall {time.time() - t0:.2f} s')
    assert not fails, '\n'.join(fails)


# ---- the many-pixel cases ---------------------------------------------------------------------------------------------------------------
# The 8-channel-pixel form has a fixed ld == 8 and the image-facing kernels are used at ld == Cb == 4: no giant stride reaches their
# limit switch, so they get real views of about 10^8 pixels, 16 bytes each, just below the limit and exactly at it (the smallest
# product that crosses: N Hb Wb 16 == L).  Integer operands from a seeded device generator, float64 reference on the device, zero
# tolerance.  The weight gradient is left out: its sums run over N Hs Ws = 2.5 10^7 terms, beyond what fp32 holds exactly.
MANY = {'below': (1024, 1023), 'at': (1024, 1024)}


def _ints(seed, lo, hi, *shape):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV, dtype=torch.float32)


def _nchw(pix, N, H, W):
    """[N H W][C] -> the NCHW view of the same memory (no copy)."""
    return pix.view(N, H, W, -1).permute(0, 3, 1, 2)


class _Many:
    def __init__(self, N, Hb, Wb, Ca, Cb, side):
        self.geom = geom = (N, Hb, Wb, Ca, Cb, 2)
        Hs, Ws = X.dims(geom)
        self.Pb, self.Ps, self.Hs, self.Ws = N * Hb * Wb, N * Hs * Ws, Hs, Ws
        self.big, self.small = _ints(1, -3, 3, self.Pb, Cb), _ints(2, -3, 3, self.Ps, Ca)
        self.Wt, self.ba, self.bb = _ints(3, -2, 2, Ca, Cb, 4, 4), _ints(4, -4, 4, Ca), _ints(5, -4, 4, Cb)
        self.ops = X.Operands(geom, _nchw(self.big, N, Hb, Wb), _nchw(self.small, N, Hs, Ws), self.Wt, self.ba, self.bb)

    def want(self, op):
        return B.to_pixels(X.to_fp32_exact(X.reference64(self.ops, op)))

    def view(self, t, role, C=None, bf=False):
        from patchgan_amd import engine as E
        N, Hb, Wb, Ca, Cb, s = self.geom
        H, W, Cv = (Hb, Wb, Cb) if role == 'big' else (self.Hs, self.Ws, Ca)
        return E.View(t.view(-1), 0, t.shape[1], N, H, W, C or Cv, bf)


def _crossing(side, nbytes):
    lim = B.limit()
    assert (nbytes < lim) == (side == 'below') and abs(nbytes - lim) <= lim // 500, (side, nbytes, lim)
    return f'{nbytes} B = L {nbytes - lim:+d}'


@pytest.mark.parametrize('side', list(MANY))
def test_many_pixels_image_facing_kernels(side):
    """big = [96, Hb, Wb] pixels of 4 fp32 channels (16 bytes): k_b2s_tapkp, k_b2s_tapk, the direct kernels in both directions and the
    generic small -> big kernel, on a view just below the limit and on one exactly at it."""
    from patchgan_amd import engine as E
    from tests.gpu_util import pack
    t0 = time.time()
    N, (Hb, Wb) = 96, MANY[side]
    m = _Many(N, Hb, Wb, 4, 4, side)
    print(f'big: {m.Pb} pixels, {_crossing(side, B.extent(m.Pb, 4, 4, 4))}')
    fails = []
    want0 = m.want(0)
    t1 = time.time()
    for name, family, algo, Ca in (('tapkp', 'tapkp', L.ALGO_AUTO, 4), ('tapk', 'tapk', L.ALGO_AUTO, 2), ('direct', 'direct', L.ALGO_DIRECT, 4)):
        cop = E.ConvOp(N, Hb, Wb, Ca, 4, 2, algo)
        sym = cop.describe(0)[0]
        assert B.family_of(sym) == family, (name, sym)
        X.budget_for(m.ops, 0, sym)
        out = _nan(m.Ps * 4).view(m.Ps, 4)
        cop.big2small(m.view(m.big, 'big'), pack(m.Wt[:Ca]), 0, m.ba[:Ca].contiguous(), 0, m.view(out, 'small', Ca), L.ACT_NONE)
        torch.cuda.synchronize()
        ok = torch.equal(out[:, :Ca], want0[:, :Ca]) and bool(out[:, Ca:].isnan().all())
        print(f'  op 0 {sym} (planned for a view below the limit): {"exact" if ok else "WRONG"}')
        if not ok:
            fails.append(f'{side} op 0 {sym}: {_diff(out[:, :Ca], want0[:, :Ca])}')
    del want0
    want1 = m.want(1)
    for algo in (L.ALGO_DIRECT, L.ALGO_AUTO):
        cop = E.ConvOp(N, Hb, Wb, 4, 4, 2, algo)
        sym = cop.describe(1)[0]
        X.budget_for(m.ops, 1, sym)
        out = _nan(m.Pb * 4).view(m.Pb, 4)
        cop.small2big(m.view(m.small, 'small'), pack(m.Wt), 0, m.bb, 0, m.view(out, 'big'), L.ACT_NONE)
        torch.cuda.synchronize()
        ok = torch.equal(out, want1)
        print(f'  op 1 {sym}: {"exact" if ok else "WRONG"}')
        if not ok:
            fails.append(f'{side} op 1 {sym}: {_diff(out, want1)}')
    print(f'  wall {time.time() - t0:.2f} s (operands and first reference {t1 - t0:.2f} s)')
    del m, want1, out
    E.release_workspaces()
    torch.cuda.empty_cache()
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('side', list(MANY))
def test_many_pixels_bf16_8_channel_pixels(side):
    """The 8-channel-pixel bf16 input of k_conv_bf16x (ld == 8, 16 bytes per pixel): just below the limit it runs and is exact; at
    the limit a bf16 tensor has no kernel -- PG_EINVAL, nothing written."""
    from patchgan_amd import engine as E
    from tests.gpu_util import pack
    t0 = time.time()
    N, (Hb, Wb), Ca = 96, MANY[side], 32
    m = _Many(N, Hb, Wb, Ca, 4, side)
    big8 = torch.zeros(m.Pb, 8, dtype=torch.bfloat16, device=DEV)
    big8[:, :4] = m.big
    print(f'big: {m.Pb} pixels of 8 bf16 channels, {_crossing(side, B.extent(m.Pb, 8, 8, 2))}')
    cop = E.ConvOp(N, Hb, Wb, Ca, 4, 2, L.ALGO_BF16)
    sym = cop.describe(0, L.IO_BIG_BF16)[0]
    out = _nan(m.Ps * Ca).view(m.Ps, Ca)
    call = lambda: cop.big2small(m.view(big8, 'big', 4, True), pack(m.Wt), 0, m.ba, 0, m.view(out, 'small'), L.ACT_NONE)
    if side == 'below':
        assert sym.startswith('k_conv_bf16x<'), sym
        X.budget_for(m.ops, 0, sym)
        call()
        torch.cuda.synchronize()
        want = m.want(0)
        ok = torch.equal(out, want)
        msg = '' if ok else _diff(out, want)
        del want
    else:
        with pytest.raises(RuntimeError, match='PG_EINVAL'):
            call()
        torch.cuda.synchronize()
        ok = bool(out.isnan().all())
        msg = 'PG_EINVAL, but the output was written'
    print(f'  op 0 {sym}: {"exact" if side == "below" else "PG_EINVAL, nothing written"}' if ok else f'  op 0 {sym}: WRONG')
    print(f'  wall {time.time() - t0:.2f} s')
    del m, big8, out
    E.release_workspaces()
    torch.cuda.empty_cache()
    assert ok, msg


@pytest.mark.parametrize('side', list(MANY))
def test_many_pixels_one_pass_transposed_conv(side):
    """k_s2b_tapnf (32 -> 4 channels): its binding operand is `small`, 128 bytes per pixel, so here `small` sits just below the limit
    and exactly at it (big: 5 10^7 pixels of 16 bytes); at the limit the planner hands the call to the row GEMM / generic kernels."""
    from patchgan_amd import engine as E
    from tests.gpu_util import pack
    t0 = time.time()
    N, (Hb, Wb), Ca = 48, MANY[side], 32
    m = _Many(N, Hb, Wb, Ca, 4, side)
    print(f'small: {m.Ps} pixels of {Ca} channels, {_crossing(side, B.extent(m.Ps, Ca, Ca, 4))}; big: {m.Pb} pixels')
    cop = E.ConvOp(N, Hb, Wb, Ca, 4, 2, L.ALGO_AUTO)
    sym = cop.describe(1)[0]
    assert B.family_of(sym) == 'tapnf', sym
    X.budget_for(m.ops, 1, sym)
    X.budget_for(m.ops, 1, B.GENERIC[1])
    out = _nan(m.Pb * 4).view(m.Pb, 4)
    cop.small2big(m.view(m.small, 'small'), pack(m.Wt), 0, m.bb, 0, m.view(out, 'big'), L.ACT_NONE)
    torch.cuda.synchronize()
    want = m.want(1)
    ok = torch.equal(out, want)
    msg = '' if ok else _diff(out, want)
    print(f'  op 1 {sym} (planned for a view below the limit): {"exact" if ok else "WRONG"}')
    print(f'  wall {time.time() - t0:.2f} s')
    del m, out, want
    E.release_workspaces()
    torch.cuda.empty_cache()
    assert ok, msg
