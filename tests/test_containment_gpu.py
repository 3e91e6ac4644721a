"""Containment: every entry point of the C ABI writes only what the caller handed it.

Three promises of include/patchgan_hip.h are held here against guarded buffers (tests/guard_util.py: all-ones bytes before, after
and between the channels of every tensor, compared byte for byte after the call):
  1. tensors are channel slices of wider buffers -- a kernel writes the slice's channels of each pixel and nothing else;
  2. the caller owns all memory and the size queries say how much -- workspaces and hand-over buffers have EXACTLY the queried
     size, and nothing beyond it changes;
  3. a smaller (or NULL) workspace is legal -- the reduced-workspace ladder runs every planner family with the claim shrunk.
Values are checked too, against torch float64 on the GPU at the bounds the per-kernel tests use for each path (a kernel that reads
the all-ones NaN next to its operands fails those).  The conv case list is a module-level function (conv_cases) built from planner
queries alone: tests/test_containment_cpu.py holds its kernel-family coverage without a GPU.  Needs an MI355X."""
import ctypes
import math
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

PG_OK, PG_EINVAL, PG_EWORKSPACE = 0, -1, -2
OPS = ('b2s', 's2b', 'wgrad')
OPCODE = {'b2s': 0, 's2b': 1, 'wgrad': 2, 'bwd': 3}

# geom = (N, Hb, Wb, Ca, Cb, stride); algo = PG_ALGO_* | PG_TUNE_*; storage: 'f32' (fp32 tensors), 'bf' (bf16 tensors), 'bf8' (bf16
# tensors, the few-channel big tensor in 8-channel pixels); src: the geometry list the case comes from
Case = namedtuple('Case', 'geom algo storage src')


def _lib():
    from patchgan_amd import _lib as L
    return L, L.load()


def conv_geom(geom):
    from patchgan_amd import _lib as L
    N, Hb, Wb, Ca, Cb, s = geom
    return L.ConvGeom(N, Hb, Wb, (Hb - 2) // s + 1, (Wb - 2) // s + 1, Ca, Cb, s)


def io_bits(storage, op):
    """PG_IO_* bits of the call: fp32 tensors none; bf16 tensors both, except small2big onto 8-channel pixels' fp32 counterpart
    (tests/test_bf16_storage_gpu.py: PG_IO_SMALL_BF16 alone, fp32 result)."""
    from patchgan_amd import _lib as L
    if storage == 'f32':
        return 0
    return L.IO_SMALL_BF16 if (storage == 'bf8' and op == 's2b') else L.IO_MASK


_WS = {}


def ws_full(geom, op):
    if (geom, op) not in _WS:
        L, lib = _lib()
        _WS[geom, op] = int(lib.pg_conv_workspace_bytes(ctypes.byref(conv_geom(geom)), OPCODE[op]))
    return _WS[geom, op]


def hand_query(case, op, hand, claim):
    """Bytes of a hand-over buffer of a call at the claimed workspace (0: the call does not take a path that has such an operand):
    part from pg_conv_stats_chunks, u from pg_conv_u_bytes, v_keep / v_pre from pg_conv_v_bytes."""
    L, lib = _lib()
    g = conv_geom(case.geom)
    a = case.algo | io_bits(case.storage, op if op != 'bwd' else 'wgrad')
    if hand == 'part':
        oc = OPCODE[op]
        return case.geom[0] * int(lib.pg_conv_stats_chunks(ctypes.byref(g), oc, a, claim)) * (g.Ca if oc == 0 else g.Cb) * 2 * 8
    if hand == 'u':
        return int(lib.pg_conv_u_bytes(ctypes.byref(g), 0 if op == 'bwd' else OPCODE[op], a, claim))
    return int(lib.pg_conv_v_bytes(ctypes.byref(g), a, claim))


def kernel_name(geom, opcode, algo_io, ws_bytes):
    """(rc, symbol) of pg_conv_kernel: the main kernel of the call the planner would launch with a workspace of ws_bytes."""
    L, lib = _lib()
    name = ctypes.create_string_buffer(192)
    s, fl = ctypes.c_int(0), ctypes.c_double(0)
    rc = lib.pg_conv_kernel(ctypes.byref(conv_geom(geom)), opcode + 16 * algo_io, ws_bytes, name, 192, ctypes.byref(s), ctypes.byref(fl))
    return rc, name.value.decode()


def family(sym):
    """Kernel family of a describe() symbol: the text before '<' (of each part of a two-launch symbol)."""
    return '+'.join(sorted({part.split('<')[0] for part in sym.split('+')}))


def families_of(case):
    """{(op, stride, family, bf16 tensors)} of the three ops of a case, planned with exactly the workspace the test passes.  An op
    whose launch on bf16 tensors is refused (expected_rc: the planner names no bf16 kernel for it) reaches no family."""
    out = set()
    for op in OPS:
        rc, sym = kernel_name(case.geom, OPCODE[op], case.algo | io_bits(case.storage, op), ws_full(case.geom, op))
        assert rc == PG_OK, (case, op, rc)
        if expected_rc(case, op, ws_full(case.geom, op)) == PG_OK:
            out.add((op, case.geom[5], family(sym), case.storage != 'f32'))
    return out


def expected_rc(case, op, claim):
    """What the header promises for the plain call (no hand-over, no dbias) with a workspace of `claim` bytes.  fp32 tensors: PG_OK.
    bf16 tensors run on bf16 kernels only, so the rule is the one the engines use (engine._bf16_tensors_ok): the call runs where
    pg_conv_kernel names a bf16 kernel for it at that workspace; where it names one only at the full workspace (the LDS-DMA kernels
    read packed weights from the workspace, and the register-staged kernels do not cover e.g. 8-channel pixels) PG_EWORKSPACE; where
    it names none at all PG_EINVAL.  Nothing is launched in the last two."""
    if case.storage == 'f32':
        return PG_OK
    ops = ('wgrad', 'b2s') if op == 'bwd' else (op,)

    def covered(ws):
        return all('bf16' in kernel_name(case.geom, OPCODE[o], case.algo | io_bits(case.storage, o), ws)[1] for o in ops)
    if covered(claim):
        return PG_OK
    return PG_EWORKSPACE if covered(ws_full(case.geom, op)) else PG_EINVAL


def colsum_floor(case):
    """Bytes of workspace below which pg_conv4x4_wgrad with dbias returns PG_EWORKSPACE (the header: 1024 * Ca floats, rounded up to 256)."""
    return (1024 * case.geom[3] * 4 + 255) // 256 * 256


def candidates():
    """Every (geometry, algo | tune bits, storage) combination the per-kernel tests use to reach each kernel family."""
    from patchgan_amd import _lib as L
    from tests import test_kernels_gpu as K, test_bf16_storage_gpu as B
    A = L.ALGO_AUTO
    out = []
    for geom in K.GEOMS:
        out += [Case(geom, algo, 'f32', 'K.GEOMS') for algo in (L.ALGO_DIRECT, L.ALGO_MFMA, L.ALGO_BF16, A)]
    for geom in K.WINO_GEOMS:
        for bits in (0, L.TUNE_WINO1_F2, L.TUNE_WINO1_F3, L.TUNE_WINO1_F3 | L.TUNE_WINO_DMA, L.TUNE_WINO1_F2 | L.TUNE_WINO_DMA, L.TUNE_S3_OFF,
                     L.TUNE_WINO1_F3 | L.TUNE_S3_OFF):
            out.append(Case(geom, A | bits, 'f32', 'K.WINO_GEOMS'))
    for geom in K.WINO2_GEOMS:
        for bits in (L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL, L.TUNE_WINO2_ALL | L.TUNE_WINO2W_ALL | L.TUNE_S3_OFF):
            out.append(Case(geom, A | bits, 'f32', 'K.WINO2_GEOMS'))
    for geom in B.GEOMS:
        out.append(Case(geom, L.ALGO_BF16 | L.TUNE_BF16X_OFF, 'bf', 'B.GEOMS'))
    for geom in B.XGEOMS:
        out += [Case(geom, L.ALGO_BF16 | bits, 'bf', 'B.XGEOMS') for bits in (L.TUNE_BF16X_FLAT, L.TUNE_BF16X_RING, L.TUNE_BF16X_OFF)]
    for geom in B.SEAMS:
        out.append(Case(geom, L.ALGO_BF16, 'bf8', 'B.SEAMS'))
    return out


def elements(case):
    N, Hb, Wb, Ca, Cb, s = case.geom
    return N * (Hb * Wb * Cb + ((Hb - 2) // s + 1) * ((Wb - 2) // s + 1) * Ca) + 16 * Ca * Cb


_REPS = []


def representatives():
    """{(op, stride, family, bf16 tensors): the candidate with the fewest elements that reaches it}."""
    if not _REPS:
        best = {}
        for c in candidates():
            for key in families_of(c):
                if key not in best or (elements(c), c) < (elements(best[key]), best[key]):
                    best[key] = c
        _REPS.append(best)
    return _REPS[0]


def conv_cases():
    """The cases of the conv containment test: one representative per (op, stride, kernel family, tensor type), each run through all its ops."""
    return sorted(set(representatives().values()), key=lambda c: (c.storage, c.geom, c.algo))


def family_ladder_cases():
    """(case, op) per kernel family for the reduced-workspace ladder."""
    return sorted(((c, key[0]) for key, c in representatives().items()), key=lambda t: (t[0].storage, t[0].geom, t[0].algo, t[1]))


def split_k_ladder_cases():
    """The smallest representatives plan one or two split-K slabs at most.  The layers of the same lists that split K deeply (small M,
    long K) ride the ladder too: the fp32 one runs 4 / 8 slabs from full / 16 upwards and one below, the bf16 one another split at
    almost every rung (pg_bf16x_clamp) and the register-staged kernels below the packed weights' size."""
    from patchgan_amd import _lib as L
    deep = [Case((2, 4, 4, 512, 64, 2), L.ALGO_MFMA, 'f32', 'K.GEOMS'), Case((2, 8, 8, 512, 512, 2), L.ALGO_BF16 | L.TUNE_BF16X_FLAT, 'bf', 'B.XGEOMS')]
    return [(c, op) for c in deep for op in ('b2s', 's2b')]        # (their weight gradients do not split, and ask for 0.1 - 1 GB)


def ladder_cases():
    return family_ladder_cases() + split_k_ladder_cases()


def case_id(c):
    if isinstance(c, tuple) and not isinstance(c, Case):
        return case_id(c[0]) + '-' + c[1]
    return 'x'.join(map(str, c.geom)) + f'-{c.algo:#x}-{c.storage}'


# ---- one conv call on guarded buffers ----------------------------------------------------------------------------------------------

class ConvCall:
    """One call of a conv entry point through the C ABI, every buffer guarded: outputs are slices (ld = C + 4 fp32 / C + 8 bf16,
    non-zero channel offset) of all-ones buffers, inputs guarded views with their own padding, dP / dbias / hand-overs guarded flat
    buffers of exactly the queried size, the workspace exactly pg_conv_workspace_bytes(g, op) with a back guard at least as large."""

    def __init__(self, case, op, T, claim=None, hand=None, hand_buf=None, epilogue=True, dbias=True, u_valid=False):
        from tests import guard_util as G
        L, lib = _lib()
        self.case, self.op, self.T, self.hand = case, op, T, hand
        N, Hb, Wb, Ca, Cb, s = case.geom
        Hs, Ws = T.Hs, T.Ws
        st = case.storage
        bf = st != 'f32'
        self.io = io_bits(st, op if op != 'bwd' else 'wgrad')
        self.algo_io = case.algo | self.io
        self.g = conv_geom(case.geom)
        self.full = ws_full(case.geom, op)
        self.claim = self.full if claim is None else claim
        assert self.claim <= self.full
        self.ws = G.flat(self.full, back=max(self.full, G.BACK))
        self.inputs = G.Inputs()
        add = self.inputs.add
        pad = (4, 4) if not bf else (8, 8)                    # (extra pixel stride, channel offset)
        epilogue = epilogue and hand != 'part'
        self.act = L.ACT_LEAKY if epilogue else L.ACT_NONE
        self.bias_g = self.bias64 = None
        self.out = self.out_g = self.dP = self.db = None
        P = T.W.permute(2, 3, 0, 1).contiguous().reshape(-1).float()
        if op in ('b2s', 'wgrad', 'bwd'):                     # `big` is an input
            if st == 'bf8':
                self.big, self.big_g = G.view_from(T.big, ld=8, off=0, bf=True, pad=0.0)
            else:
                self.big, self.big_g = G.view_from(T.big, ld=Cb + pad[0], off=0 if not bf else 8, bf=bf)
            add(self.big_g, 'big')
        if op in ('s2b', 'wgrad', 'bwd'):                     # `small` is an input
            self.small, self.small_g = G.view_from(T.small, ld=Ca + pad[0], off=pad[1], bf=bf)
            add(self.small_g, 'small')
        if op != 'wgrad':
            self.P_g = add(G.flat_from(P), 'P')
        if op == 'b2s':
            self.out, self.out_g = G.view(N, Hs, Ws, Ca, ld=Ca + pad[0], off=pad[1], bf=bf)
            if epilogue:
                self.bias64, self.bias_g = T.bias_a, add(G.flat_from(T.bias_a.float()), 'bias')
        elif op == 's2b':
            out_bf = bool(self.io & L.IO_BIG_BF16)
            self.out, self.out_g = G.view(N, Hb, Wb, Cb, ld=Cb + (8 if out_bf else 4), off=8 if out_bf else 4, bf=out_bf)
            if epilogue:
                self.bias64, self.bias_g = T.bias_b, add(G.flat_from(T.bias_b.float()), 'bias')
        else:
            self.dP = G.flat(16 * Ca * Cb * 4)
            if op == 'wgrad' and dbias and (not bf or Ca % 4 == 0):
                self.db = G.flat(Ca * 4)
            if op == 'bwd':
                self.out, self.out_g = G.view(N, Hs, Ws, Ca, ld=Ca + pad[0], off=pad[1], bf=bf)
        # the hand-over of this call: a guarded flat buffer of exactly the queried size (hand_buf: one filled by an earlier call)
        self.hand_g, self.hand_bytes = hand_buf, 0
        if hand is not None:
            self.hand_bytes = self.query(hand)
            if hand_buf is None and self.hand_bytes:
                self.hand_g = G.flat(self.hand_bytes)
            elif hand_buf is None:
                # a probe (the query says 0: the call must refuse it).  Should the library take it after all, what it writes -- an
                # operand that otherwise lives in the workspace, or a few partial sums per pixel tile -- lands in this buffer's back guard
                self.hand_g = G.flat(4096, back=ws_full(case.geom, op) + (1 << 20))
            if hand == 'v_pre' or u_valid:
                add(self.hand_g, hand)
        self.u_valid = u_valid
        self.rc = None

    def query(self, hand):
        return hand_query(self.case, self.op, hand, self.claim)

    def run(self):
        L, lib = _lib()
        wp = self.ws.ptr() if self.claim else None
        x = None
        if self.hand is not None:
            hp = self.hand_g.ptr()
            x = L.ConvExtras(hp if self.hand == 'part' else None, hp if self.hand == 'v_keep' else None, hp if self.hand == 'v_pre' else None,
                             hp if self.hand == 'u' else None, 1 if self.u_valid else 0, None, 0, 0)
        xr = (ctypes.byref(x),) if x is not None else ()
        g = ctypes.byref(self.g)
        bp = self.bias_g.ptr() if self.bias_g is not None else None
        if self.op == 'b2s':
            fn = lib.pg_conv4x4_big2small_x if x is not None else lib.pg_conv4x4_big2small
            self.rc = fn(self.big.ptr(), self.big.ld, self.P_g.ptr(), bp, self.out.ptr(), self.out.ld, g, self.act, self.algo_io, wp, self.claim, None, *xr)
        elif self.op == 's2b':
            fn = lib.pg_conv4x4_small2big_x if x is not None else lib.pg_conv4x4_small2big
            self.rc = fn(self.small.ptr(), self.small.ld, self.P_g.ptr(), bp, self.out.ptr(), self.out.ld, g, self.act, self.algo_io, wp, self.claim, None, *xr)
        elif self.op == 'wgrad':
            fn = lib.pg_conv4x4_wgrad_x if x is not None else lib.pg_conv4x4_wgrad
            self.rc = fn(self.small.ptr(), self.small.ld, self.big.ptr(), self.big.ld, self.dP.ptr(), self.db.ptr() if self.db is not None else None, g,
                         self.algo_io, wp, self.claim, None, *xr)
        else:
            fn = lib.pg_conv4x4_bwd_big_x if x is not None else lib.pg_conv4x4_bwd_big
            self.rc = fn(self.small.ptr(), self.small.ld, self.big.ptr(), self.big.ld, self.P_g.ptr(), self.dP.ptr(), self.out.ptr(), self.out.ld, g,
                         self.algo_io, wp, self.claim, None, *xr)
        torch.cuda.synchronize()
        return self.rc

    def what(self):
        return f'{case_id(self.case)} {self.op} ws {self.claim}/{self.full}' + (f' {self.hand}' if self.hand else '')

    def check_nothing_written(self):
        """A refused call launched nothing: every buffer is as it was."""
        from tests import guard_util as G
        w = self.what() + f' rc {self.rc}'
        for g, name in ((self.out_g, 'output'), (self.dP, 'dP'), (self.db, 'dbias'), (self.ws, 'workspace')):
            if g is not None:
                G.assert_untouched(g, None, f'{w} {name}')
        if self.hand_g is not None and not (self.hand == 'v_pre' or self.u_valid):
            G.assert_untouched(self.hand_g, None, f'{w} {self.hand}')
        self.inputs.check(w)

    def check_written(self):
        """After PG_OK: values against float64, nothing outside the output slice / dP / dbias / the first `claim` bytes of the workspace /
        the queried bytes of the hand-over changed, inputs byte-identical."""
        from tests import guard_util as G
        w = self.what()
        self.check_values()
        if self.out_g is not None:
            G.assert_untouched(self.out_g, 'slice', w + ' output')
        if self.dP is not None:
            G.assert_untouched(self.dP, 'all', w + ' dP')
        if self.db is not None:
            G.assert_untouched(self.db, 'all', w + ' dbias')
        G.assert_untouched(self.ws, self.claim, w + ' workspace')
        if self.hand_g is not None and not (self.hand == 'v_pre' or self.u_valid):
            G.assert_untouched(self.hand_g, self.hand_bytes, f'{w} {self.hand}')
        self.inputs.check(w)

    def check_values(self):
        from tests import guard_util as G
        case, T, w = self.case, self.T, self.what()
        Ca, Cb = case.geom[3], case.geom[4]
        tol_f, tol_w = tolerances(case)
        if self.op in ('b2s', 's2b'):
            lin = T.ref(self.op)
            if self.bias64 is not None:
                lin = lin + self.bias64.view(1, -1, 1, 1)
            want = torch.where(lin > 0, lin, lin * 0.2) if self.act else lin
            check_tensor(G.read_nchw(self.out), want, self.out.bf, tol_f, case, w)
        else:
            dP = self.dP.inner(torch.float32).view(4, 4, Ca, Cb).permute(2, 3, 0, 1).double()
            check_tensor(dP, T.ref('wgrad'), False, tol_w, case, w + ' dP')
            if self.db is not None:         # (the bias gradient is an fp32 column sum under every algo: 3e-5 as test_wgrad, 2e-5 from bf16 dy)
                check_tensor(self.db.inner(torch.float32).double(), T.small.sum((0, 2, 3)), False, 3e-5 if case.storage == 'f32' else 2e-5, case,
                             w + ' dbias')
            if self.op == 'bwd':
                check_tensor(G.read_nchw(self.out), T.ref('b2s'), self.out.bf, tol_f, case, w + ' dsmall')
        if self.hand == 'part' and self.hand_bytes:
            assert not torch.isnan(self.hand_g.inner(torch.float64)).any().item(), w + ': partial sums not all written'


def tolerances(case):
    """(forward / data gradient, weight gradient) bounds in relative max-norm against float64, those of the per-kernel tests:
    fp32 kernels 2e-5 / 3e-5; PG_ALGO_BF16 on fp32 tensors 2e-2; bf16 tensors as tests/test_bf16_storage_gpu.py -- its GEOMS list
    (register-staged kernels) 2e-2, its XGEOMS / SEAMS lists (operands and weights bf16-representable) 2e-5."""
    if case.storage == 'f32':
        return (2e-2, 2e-2) if (case.algo & 0xF) == 3 else (2e-5, 3e-5)
    return (2e-2, 2e-2) if case.src == 'B.GEOMS' else (2e-5, 2e-5)


def check_tensor(got64, want64, out_bf, tol, case, what):
    scale = want64.abs().max().item()
    assert math.isfinite(scale) and scale > 0, what
    if out_bf and tol <= 2e-5:              # within one bf16 ulp of the rounded float64 value (test_lds_dma_bf16_kernels)
        ref = want64.float().bfloat16().double()
        bad = ~((got64 - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-5 * scale)
        assert not bad.any().item(), (what, 'beyond one bf16 ulp', ((got64 - ref).abs().max() / scale).item())
    elif out_bf:                            # the fp32 kernel's bound plus the rounding of the stored value (half a bf16 ulp = 2^-9 relative)
        bad = ~((got64 - want64).abs() <= want64.abs() * 2.0 ** -8 + tol * scale)
        assert not bad.any().item(), (what, ((got64 - want64).abs().max() / scale).item())
    else:
        err = ((got64 - want64).abs().max() / scale).item()
        assert err < tol, (what, err, tol)          # (a NaN read from a guard makes err NaN: fails)


def _truth(case):
    from tests.test_bench_layers_gpu import _get_truth
    return _get_truth(case.geom, case.storage != 'f32')


def _ops_of(case):
    return OPS + (('bwd',) if case.geom[5] == 2 else ())


def _run_ok(call):
    """Runs the call and holds it to the promised return code: PG_OK with a hand-over that the size query sized, else expected_rc
    (the dbias floor is the ladder's own business).  True: it ran and stayed inside its buffers; False: refused, nothing written."""
    rc = call.run()
    want = PG_OK if call.hand else expected_rc(call.case, call.op, call.claim)
    assert rc == want, (call.what(), rc, want)
    if rc == PG_OK:
        call.check_written()
        return True
    call.check_nothing_written()
    return False


@pytest.mark.parametrize('case', conv_cases(), ids=case_id)
def test_conv_calls_stay_inside_their_buffers(case):
    """The three ops (and pg_conv4x4_bwd_big on stride 2) of one representative per kernel family, workspace and hand-overs of
    exactly the queried size.  Every op the case represents a family for must run (PG_OK); an op that bf16 tensors have no kernel for
    must be refused with exactly PG_EINVAL and nothing written."""
    T = _truth(case)
    ran = set()
    for op in _ops_of(case):
        if _run_ok(ConvCall(case, op, T)):
            ran.add(op)
        # the hand-overs this call has at the full workspace: part (no bias / activation), u_cache (filled, then read), v_keep -> v_pre
        if op in ('b2s', 's2b'):
            c = ConvCall(case, op, T, hand='part')
            if c.hand_bytes:
                _run_ok(c)
        if op != 'wgrad':
            c = ConvCall(case, op, T, hand='u')
            if c.hand_bytes and _run_ok(c):
                c2 = ConvCall(case, op, T, hand='u', hand_buf=c.hand_g, u_valid=True)
                c2.hand_bytes = c.hand_bytes
                _run_ok(c2)
        if op == 'b2s':
            c = ConvCall(case, op, T, hand='v_keep')
            if c.hand_bytes and hand_query(case, 'wgrad', 'v_pre', ws_full(case.geom, 'wgrad')) and _run_ok(c):
                _run_ok(ConvCall(case, 'wgrad', T, hand='v_pre', hand_buf=c.hand_g))      # (its snapshot of V is taken after the forward call)
    assert ran >= {key[0] for key, c in representatives().items() if c == case}, (case, ran)


def _rungs(full):
    """NULL / 0, 256 B, full / 16, full / 2, full - 256 and full, each rounded down to a multiple of 256, duplicates dropped."""
    out = []
    for r in (0, 256, full // 16, full // 2, full - 256, full):
        r = max(r, 0) // 256 * 256
        if r <= full and r not in out:
            out.append(r)
    return out


@pytest.mark.parametrize('case_op', ladder_cases(), ids=case_id)
def test_reduced_workspace_ladder(case_op):
    """The same call with the workspace CLAIM shrunk (the buffer stays full + guard).  PG_OK -- then the output is within the float64
    bounds of the full-size call and nothing beyond the claimed bytes of the workspace changed -- or PG_EWORKSPACE with nothing
    launched; PG_OK at the full size and, with no dbias and no hand-overs, at NULL.  The two documented exceptions are asserted
    exactly: the weight gradient with dbias is refused below colsum_floor and runs from there on; a bf16-tensor call that only the
    LDS-DMA kernels cover is PG_EWORKSPACE where expected_rc says so.  A hand-over whose size query says 0 at the claimed size is
    refused with PG_EINVAL, nothing launched; one the query sizes is passed at exactly that size."""
    from tests import guard_util as G
    case, op = case_op
    T = _truth(case)
    full = ws_full(case.geom, op)
    assert expected_rc(case, op, full) == PG_OK, (case, op)          # (a ladder case is one whose own launch runs)
    variants = [dict()] if op != 'wgrad' else [dict(dbias=False), dict(dbias=True)]
    hands = {'b2s': ('part', 'u', 'v_keep'), 's2b': ('part', 'u'), 'wgrad': ('v_pre',)}[op]
    bf = case.storage != 'f32'
    spare = {}                  # hand-over buffers of refused calls (still all sentinel: asserted), reused on the next rung
    for claim in _rungs(full):
        rc, sym = kernel_name(case.geom, OPCODE[op], case.algo | io_bits(case.storage, op), claim)
        assert rc == PG_OK, (case, op, claim, rc)
        if claim == 0:
            assert 'k_wino' not in sym, (case, op, sym)
        for kw in variants:
            call = ConvCall(case, op, T, claim=claim, **kw)
            rc = call.run()
            w = (call.what(), kw, rc, sym)
            assert rc in (PG_OK, PG_EWORKSPACE), w
            if call.db is not None and claim < colsum_floor(case):
                assert rc == PG_EWORKSPACE, w
            elif bf or call.db is not None:
                assert rc == expected_rc(case, op, claim), w
            elif claim == full or claim == 0:
                assert rc == PG_OK, w
            call.check_written() if rc == PG_OK else call.check_nothing_written()
        for hand in hands:
            nb = hand_query(case, op, hand, claim)
            if nb and hand != 'v_pre':          # the path has this operand at the claimed size: a buffer of exactly that size
                _run_ok(ConvCall(case, op, T, claim=claim, hand=hand))
            if nb:
                continue                        # (v_pre needs the forward call's V: run at the full size in the test above)
            # with the bias gradient at the full size, too: a refused call must not have started its column sums
            probe = ConvCall(case, op, T, claim=claim, hand=hand, hand_buf=spare.get(hand), dbias=claim == full)
            rc = probe.run()
            assert rc == PG_EINVAL, (probe.what(), rc, 'a hand-over the size query reports 0 bytes for must be refused')
            probe.check_nothing_written()
            G.assert_untouched(probe.hand_g, None, probe.what())
            spare[hand] = probe.hand_g


# ---- norm kernels ------------------------------------------------------------------------------------------------------------------

def _norm_ref(y64, act):
    m = y64.mean((2, 3), keepdim=True)
    v = y64.var((2, 3), unbiased=False, keepdim=True)
    o = (y64 - m) / torch.sqrt(v + 1e-5)
    return torch.where(o > 0, o, o * 0.2) if act == 1 else o


def _rel(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize('wsmode', ['exact', 'null', 'short'])
@pytest.mark.parametrize('mix', ['all_fp32', 'all_bf16', 'y32_out16', 'g16_y32_dy32'])
@pytest.mark.parametrize('shape', [(3, 6, 5, 7), (2, 8, 16, 32), (2, 64, 23, 23)], ids=lambda s: 'x'.join(map(str, s)))
def test_instnorm_chunked_and_fallback_paths(shape, mix, wsmode):
    """pg_instnorm_act_fwd / _bwd (all_fp32) and their _t forms (the three storage mixes of test_instnorm_act_mixed_storage) on the
    scalar path (C % 4 != 0), the smallest plane the chunk plan splits (HW = 512; not for all_bf16, whose 8 channels are one 16-byte unit
    there: one chunk, the one-workgroup kernels -- tests/test_normact_gpu.py has the smallest split bf16 plane, C = 16) and a ragged last
    chunk (HW = 529), with a workspace
    of exactly pg_instnorm_workspace_bytes, NULL, and one 256-byte step too small (the last two: the one-workgroup fallback).  Against
    float64 autograd: 1e-5 forward, 5e-5 backward (fp32 results; bf16 results within one bf16 ulp of the rounded value, inputs
    bf16-representable)."""
    from tests import guard_util as G
    L, lib = _lib()
    N, C, H, W = shape
    gen = torch.Generator(device='cuda').manual_seed(1)
    rnd = lambda: torch.randn(shape, device='cuda', generator=gen).bfloat16().double()
    y = (rnd() * 2 + 0.5).float().bfloat16().double().requires_grad_(True)
    g1, g2 = rnd(), rnd()
    want = _norm_ref(y, 1)
    want.backward(g1 + g2)
    y_bf = mix == 'all_bf16'
    out_bf = mix in ('all_bf16', 'y32_out16')
    g_bf = mix in ('all_bf16', 'g16_y32_dy32')
    dy_bf = mix == 'all_bf16'
    pad = lambda bf: dict(ld=C + (8 if bf else 4), off=8 if bf else 4, bf=bf)
    full = int(lib.pg_instnorm_workspace_bytes(N, H * W, C))
    claim = {'exact': full, 'null': 0, 'short': max(full - 256, 0)}[wsmode]
    ins = G.Inputs()
    vy, gy = G.view_from(y.detach(), **pad(y_bf))
    ins.add(gy, 'y')
    vo, go = G.view(N, H, W, C, **pad(out_bf))
    stats = G.flat(N * C * 2 * 4)
    ws = G.flat(full, back=max(full, G.BACK))
    wp = ws.ptr() if wsmode != 'null' else None
    dt = (1 if y_bf else 0) | (2 if out_bf else 0)
    if mix == 'all_fp32':
        rc = lib.pg_instnorm_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, stats.ptr(), N, H * W, C, 1, 1e-5, 0.0, 0, wp, claim, None)
    else:
        rc = lib.pg_instnorm_act_fwd_t(vy.ptr(), vy.ld, vo.ptr(), vo.ld, stats.ptr(), N, H * W, C, 1, 1e-5, 0.0, 0, wp, claim, None, dt)
    torch.cuda.synchronize()
    assert rc == PG_OK
    what = f'instnorm fwd {shape} {mix} ws {claim}/{full}'
    _check_norm(G.read_nchw(vo), want.detach(), out_bf, 1e-5, what)
    G.assert_untouched(go, 'slice', what + ' out')
    G.assert_untouched(stats, 'all', what + ' stats')
    G.assert_untouched(ws, claim, what + ' workspace')
    ins.check(what)
    st = stats.inner(torch.float32).view(N, C, 2).double()
    assert _rel(st[..., 0], y.detach().mean((2, 3))) < 1e-5, what
    # backward
    vg1, gg1 = G.view_from(g1, **pad(g_bf))
    vg2, gg2 = G.view_from(g2, **pad(g_bf))
    ins.add(gg1, 'g1'), ins.add(gg2, 'g2'), ins.add(stats, 'stats')
    vd, gd = G.view(N, H, W, C, **pad(dy_bf))
    ws2 = G.flat(full, back=max(full, G.BACK))
    wp = ws2.ptr() if wsmode != 'null' else None
    dt = (1 if g_bf else 0) | (2 if g_bf else 0) | (4 if y_bf else 0) | (8 if dy_bf else 0)
    if mix == 'all_fp32':
        rc = lib.pg_instnorm_act_bwd(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, stats.ptr(), vd.ptr(), vd.ld, N, H * W, C, 1, 0.0, 0,
                                     wp, claim, None)
    else:
        rc = lib.pg_instnorm_act_bwd_t(vg1.ptr(), vg1.ld, vg2.ptr(), vg2.ld, vy.ptr(), vy.ld, stats.ptr(), vd.ptr(), vd.ld, N, H * W, C, 1, 0.0, 0,
                                       wp, claim, None, dt)
    torch.cuda.synchronize()
    assert rc == PG_OK
    what = f'instnorm bwd {shape} {mix} ws {claim}/{full}'
    _check_norm(G.read_nchw(vd), y.grad, dy_bf, 5e-5, what)
    G.assert_untouched(gd, 'slice', what + ' dy')
    G.assert_untouched(ws2, claim, what + ' workspace')
    ins.check(what)


def _check_norm(got, want, out_bf, tol, what):
    scale = want.abs().max().item()
    if out_bf:
        ref = want.float().bfloat16().double()
        bad = ~((got - ref).abs() <= ref.abs() * 2.0 ** -7 + tol * scale)
        assert not bad.any().item(), (what, ((got - ref).abs().max() / scale).item())
    else:
        err = ((got - want).abs().max() / scale).item()
        assert err < tol, (what, err, tol)


def test_instnorm_from_conv_partials():
    """pg_instnorm_act_fwd_parts with a guarded `part` written by a conv call (the polyphase Winograd epilogue) of exactly the queried
    size: the conv writes all of it and nothing else, the norm reads it unchanged and writes only its slice and N*C*2 statistics."""
    from tests import guard_util as G
    L, lib = _lib()
    cands = [c for c in conv_cases() if c.storage == 'f32']
    picked = None
    for c in sorted(cands, key=elements):
        if hand_query(c, 'b2s', 'part', ws_full(c.geom, 'b2s')):
            picked = ConvCall(c, 'b2s', _truth(c), hand='part')
            break
    assert picked is not None, 'no fp32 case emits InstanceNorm partials'
    assert _run_ok(picked)
    N, Hb, Wb, Ca, Cb, s = picked.case.geom
    Hs, Ws = picked.T.Hs, picked.T.Ws
    chunks = picked.hand_bytes // (N * Ca * 16)
    ins = G.Inputs()
    ins.add(picked.hand_g, 'part'), ins.add(picked.out_g, 'y')
    vo, go = G.view(N, Hs, Ws, Ca, ld=Ca + 4, off=4)
    stats = G.flat(N * Ca * 2 * 4)
    rc = lib.pg_instnorm_act_fwd_parts(picked.out.ptr(), picked.out.ld, vo.ptr(), vo.ld, stats.ptr(), picked.hand_g.ptr(), chunks, N, Hs * Ws, Ca,
                                       1, 1e-5, 0.0, 0, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    what = f'instnorm_act_fwd_parts after {picked.what()}'
    _check_norm(G.read_nchw(vo), _norm_ref(G.read_nchw(picked.out), 1), False, 1e-5, what)
    G.assert_untouched(go, 'slice', what + ' out')
    G.assert_untouched(stats, 'all', what + ' stats')
    ins.check(what)


@pytest.mark.parametrize('nseg', [1, 2])
@pytest.mark.parametrize('shape', [(4, 8, 4, 4), (4, 64, 23, 23)], ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_entry_points(shape, nseg):
    """pg_batchnorm_act_fwd / _stats / _act_apply / _act_bwd / _update_running with exact workspaces and guarded coef, bstat,
    dweight, dbias and running buffers; one 256-byte step too small returns PG_EWORKSPACE with nothing written (the header: the
    BatchNorm entry points do not fall back).  Values against float64 autograd at the bounds of tests/test_batchnorm_gpu.py's
    per-kernel test (1e-5 forward, 5e-5 backward)."""
    from tests import guard_util as G
    L, lib = _lib()
    N, C, H, W = shape
    HW = H * W
    gen = torch.Generator(device='cuda').manual_seed(2)
    y = (torch.randn(shape, device='cuda', generator=gen, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    wt = (torch.rand(C, device='cuda', generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
    bs = torch.randn(C, device='cuda', generator=gen, dtype=torch.float64).requires_grad_(True)
    g1 = torch.randn(shape, device='cuda', generator=gen, dtype=torch.float64)
    seg = N // nseg
    outs = []
    for s in range(nseg):
        ys = y[s * seg:(s + 1) * seg]
        m, v = ys.mean((0, 2, 3), keepdim=True), ys.var((0, 2, 3), unbiased=False, keepdim=True)
        o = (ys - m) / torch.sqrt(v + 1e-5) * wt.view(1, -1, 1, 1) + bs.view(1, -1, 1, 1)
        outs.append(torch.where(o > 0, o, o * 0.2))
    want = torch.cat(outs)
    want.backward(g1)
    full = int(lib.pg_batchnorm_workspace_bytes(N, HW, C, nseg))
    assert full >= 256

    def operands():
        ins = G.Inputs()
        vy, gy = G.view_from(y.detach(), ld=C + 4, off=0)
        ins.add(gy, 'y')
        w_g, b_g = ins.add(G.flat_from(wt.detach().float()), 'weight'), ins.add(G.flat_from(bs.detach().float()), 'bias')
        return ins, vy, w_g, b_g

    for claim in (full - 256, full):
        ins, vy, w_g, b_g = operands()
        vo, go = G.view(N, H, W, C, ld=C + 4, off=4)
        coef, bstat = G.flat(nseg * C * 4 * 4), G.flat(nseg * C * 2 * 8)
        ws = G.flat(full, back=max(full, G.BACK))
        rc = lib.pg_batchnorm_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, w_g.ptr(), b_g.ptr(), coef.ptr(), bstat.ptr(), N, HW, C, nseg, 1, 1e-5, 0.0, 0,
                                      ws.ptr(), claim, None)
        torch.cuda.synchronize()
        what = f'batchnorm_act_fwd {shape} nseg {nseg} ws {claim}/{full}'
        if claim < full:
            assert rc == PG_EWORKSPACE, (what, rc)
            for g in (go, coef, bstat, ws):
                G.assert_untouched(g, None, what)
            ins.check(what)
            continue
        assert rc == PG_OK, (what, rc)
        assert _rel(G.read_nchw(vo), want.detach()) < 1e-5, what
        G.assert_untouched(go, 'slice', what + ' out')
        G.assert_untouched(coef, 'all', what + ' coef')
        G.assert_untouched(bstat, 'all', what + ' bstat')
        G.assert_untouched(ws, claim, what + ' workspace')
        ins.check(what)
    # the two halves: statistics (from y), then apply -- the same results
    ins, vy, w_g, b_g = operands()
    coef2, bstat2 = G.flat(nseg * C * 4 * 4), G.flat(nseg * C * 2 * 8)
    ws = G.flat(full, back=max(full, G.BACK))
    what = f'batchnorm_stats {shape} nseg {nseg}'
    rc = lib.pg_batchnorm_stats(vy.ptr(), vy.ld, None, 0, w_g.ptr(), b_g.ptr(), coef2.ptr(), bstat2.ptr(), N, HW, C, nseg, 1e-5, ws.ptr(), full - 256, None)
    torch.cuda.synchronize()
    assert rc == PG_EWORKSPACE, (what, rc)
    for g in (coef2, bstat2, ws):
        G.assert_untouched(g, None, what + ' refused')
    rc = lib.pg_batchnorm_stats(vy.ptr(), vy.ld, None, 0, w_g.ptr(), b_g.ptr(), coef2.ptr(), bstat2.ptr(), N, HW, C, nseg, 1e-5, ws.ptr(), full, None)
    torch.cuda.synchronize()
    assert rc == PG_OK, (what, rc)
    assert _rel(coef2.inner(torch.float32), coef.inner(torch.float32)) < 1e-6 and _rel(bstat2.inner(torch.float64), bstat.inner(torch.float64)) < 1e-12, what
    G.assert_untouched(coef2, 'all', what), G.assert_untouched(bstat2, 'all', what), G.assert_untouched(ws, full, what)
    ins.add(coef2, 'coef')
    vo2, go2 = G.view(N, H, W, C, ld=C + 4, off=4)
    rc = lib.pg_batchnorm_act_apply(vy.ptr(), vy.ld, vo2.ptr(), vo2.ld, coef2.ptr(), N, HW, C, nseg, 1, 0.0, 0, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    assert _rel(G.read_nchw(vo2), G.read_nchw(vo)) < 1e-6, 'batchnorm_act_apply differs from batchnorm_act_fwd'
    G.assert_untouched(go2, 'slice', 'batchnorm_act_apply out')
    ins.check('batchnorm_stats / _act_apply')
    # backward
    for claim in (full - 256, full):
        ins, vy, w_g, b_g = operands()
        ins.add(coef, 'coef')
        vg, gg = G.view_from(g1, ld=C + 4, off=4)
        ins.add(gg, 'g1')
        vd, gd = G.view(N, H, W, C, ld=C + 4, off=4)
        dw, db = G.flat(C * 4), G.flat(C * 4)
        ws = G.flat(full, back=max(full, G.BACK))
        rc = lib.pg_batchnorm_act_bwd(vg.ptr(), vg.ld, None, 0, vy.ptr(), vy.ld, coef.ptr(), vd.ptr(), vd.ld, dw.ptr(), db.ptr(), N, HW, C, nseg, 1, 1,
                                      0.0, 0, ws.ptr(), claim, None)
        torch.cuda.synchronize()
        what = f'batchnorm_act_bwd {shape} nseg {nseg} ws {claim}/{full}'
        if claim < full:
            assert rc == PG_EWORKSPACE, (what, rc)
            for g in (gd, dw, db, ws):
                G.assert_untouched(g, None, what)
            ins.check(what)
            continue
        assert rc == PG_OK, (what, rc)
        assert _rel(G.read_nchw(vd), y.grad) < 5e-5, what
        assert _rel(dw.inner(torch.float32), wt.grad) < 5e-5 and _rel(db.inner(torch.float32), bs.grad) < 5e-5, what
        G.assert_untouched(gd, 'slice', what + ' dy')
        G.assert_untouched(dw, 'all', what + ' dweight'), G.assert_untouched(db, 'all', what + ' dbias')
        G.assert_untouched(ws, claim, what + ' workspace')
        ins.check(what)
    # running statistics: nseg slots folded in slot order, the counter += nseg
    ins = G.Inputs()
    ins.add(bstat, 'bstat')
    rm, rv = G.flat_from(torch.zeros(C)), G.flat_from(torch.ones(C))
    nbt = G.flat_from(torch.zeros(1, dtype=torch.int64))
    items = (L.BnUpdateItem * 1)()
    items[0].bstat, items[0].running_mean, items[0].running_var, items[0].num_batches_tracked, items[0].C = bstat.ptr(), rm.ptr(), rv.ptr(), nbt.ptr(), C
    rc = lib.pg_batchnorm_update_running(1, items, nseg, 0.1, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    erm, erv = torch.zeros(C, dtype=torch.float64, device='cuda'), torch.ones(C, dtype=torch.float64, device='cuda')
    bsv = bstat.inner(torch.float64).view(nseg, C, 2)
    for s in range(nseg):
        erm = (0.9 * erm + 0.1 * bsv[s, :, 0]).float().double()
        erv = (0.9 * erv + 0.1 * bsv[s, :, 1]).float().double()
    assert (rm.inner(torch.float32).double() - erm).abs().max().item() < 1e-6 and _rel(rv.inner(torch.float32), erv) < 1e-6
    assert nbt.inner(torch.int64).item() == nseg
    for g in (rm, rv, nbt):
        G.assert_untouched(g, 'all', 'batchnorm_update_running')
    ins.check('batchnorm_update_running')


# ---- everything else that writes memory --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [1, 3, 8])
@pytest.mark.parametrize('bf', [False, True], ids=['fp32', 'bf16'])
def test_act_fwd_bwd_containment(C, bf):
    from tests import guard_util as G
    L, lib = _lib()
    N, H, W = 2, 6, 5
    x = torch.randn(N, C, H, W, device='cuda').bfloat16().float()
    pad = dict(ld=C + (8 if bf else 3), off=8 if bf else 1, bf=bf)
    ins = G.Inputs()
    vy, gy = G.view_from(x, **pad)
    ins.add(gy, 'y')
    vo, go = G.view(N, H, W, C, **pad)
    if bf:
        rc = lib.pg_act_fwd_t(vy.ptr(), vy.ld, vo.ptr(), vo.ld, vy.npix, C, 3, 0.0, 0, None, 3)
    else:
        rc = lib.pg_act_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, vy.npix, C, 3, 0.0, 0, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    G.assert_untouched(go, 'slice', f'act_fwd C={C}')
    assert not torch.isnan(G.read_nchw(vo)).any().item()
    ins.add(go, 'a')
    vg, gg = G.view_from(x * 0.5, **pad)
    ins.add(gg, 'g1')
    vd, gd = G.view(N, H, W, C, **pad)
    if bf:
        rc = lib.pg_act_bwd_t(vg.ptr(), vg.ld, None, 0, vo.ptr(), vo.ld, vd.ptr(), vd.ld, vy.npix, C, 3, 0.0, 0, None, 1 | 4 | 8)
    else:
        rc = lib.pg_act_bwd(vg.ptr(), vg.ld, None, 0, vo.ptr(), vo.ld, vd.ptr(), vd.ld, vy.npix, C, 3, 0.0, 0, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    G.assert_untouched(gd, 'slice', f'act_bwd C={C}')
    assert not torch.isnan(G.read_nchw(vd)).any().item()
    ins.check(f'act C={C}')


@pytest.mark.parametrize('C', [2, 7])
def test_softmax_containment(C):
    from tests import guard_util as G
    L, lib = _lib()
    N, H, W = 2, 9, 4
    x = torch.randn(N, C, H, W, device='cuda') * 3
    ins = G.Inputs()
    vy, gy = G.view_from(x, ld=8, off=1)
    ins.add(gy, 'y')
    vo, go = G.view(N, H, W, C, ld=8, off=1 if C == 7 else 3)
    assert lib.pg_softmax_fwd(vy.ptr(), vy.ld, vo.ptr(), vo.ld, vy.npix, C, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(go, 'slice', f'softmax_fwd C={C}')
    assert _rel(G.read_nchw(vo), torch.softmax(x.double(), 1)) < 1e-6
    ins.add(go, 'out')
    vg, gg = G.view_from(x * 0.25, ld=8, off=0)
    ins.add(gg, 'g1')
    vd, gd = G.view(N, H, W, C, ld=8, off=1)
    assert lib.pg_softmax_bwd(vg.ptr(), vg.ld, None, 0, vo.ptr(), vo.ld, vd.ptr(), vd.ld, vy.npix, C, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gd, 'slice', f'softmax_bwd C={C}')
    assert not torch.isnan(G.read_nchw(vd)).any().item()
    ins.check(f'softmax C={C}')


def test_dropout_mask_containment():
    from tests import guard_util as G
    L, lib = _lib()
    n = 2 * 7 * 9 * 5 + 3
    m = G.flat(n * 4)
    assert lib.pg_dropout_mask(m.ptr(), n, 0.2, 0xABCDEF12345, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(m, 'all', 'dropout_mask')
    v = m.inner(torch.float32)
    assert bool(((v == 0) | (v == 1)).all().item())


@pytest.mark.parametrize('shape', [(3, 4, 64, 80), (16, 1, 256, 256)], ids=lambda s: 'x'.join(map(str, s)))
def test_loss_kernels_containment(shape):
    """pg_loss_reduce / _reduce_parts into S of exactly pg_loss_reduce_doubles doubles (the second shape splits the reduction: the
    scratch behind the N*C*5 results is in use), pg_loss_grad and pg_loss_value_grad with the gradient into a slice of ld = C + 3."""
    from tests import guard_util as G
    L, lib = _lib()
    N, C, H, W = shape
    HW = H * W
    gen = torch.Generator(device='cuda').manual_seed(9)
    p = torch.rand(shape, device='cuda', generator=gen).clamp(1e-4, 1 - 1e-4)
    y = (torch.rand(shape, device='cuda', generator=gen) > 0.7).float()
    ins = G.Inputs()
    vp, gp = G.view_from(p, ld=C + 3, off=1)
    vy, gy = G.view_from(y, ld=C + 1, off=0)
    ins.add(gp, 'p'), ins.add(gy, 'y')
    nd = int(lib.pg_loss_reduce_doubles(N, HW, C))
    S = G.flat(nd * 8)
    assert lib.pg_loss_reduce(vp.ptr(), vp.ld, vy.ptr(), vy.ld, 1.0, N, HW, C, S.ptr(), None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(S, 'all', 'loss_reduce S')
    got = S.inner(torch.float64)[:N * C * 5].view(N, C, 5)
    pd, yd = p.double(), y.double()
    assert _rel(got[..., 0], (pd * yd).sum((2, 3))) < 1e-6 and _rel(got[..., 2], pd.sum((2, 3))) < 1e-6
    S2 = G.flat(nd * 8)
    ns = lib.pg_loss_reduce_parts(vp.ptr(), vp.ld, vy.ptr(), vy.ld, 1.0, N, HW, C, S2.ptr(), None)
    torch.cuda.synchronize()
    assert ns >= 1 and (shape[0] != 16 or ns > 1)
    G.assert_untouched(S2, 'all', 'loss_reduce_parts S')
    ins.add(S2, 'Spart')
    # value + gradient in one launch; the gradient is a slice of a wider buffer
    vg, gg = G.view(N, H, W, C, ld=C + 3, off=2)
    Sout, loss = G.flat(N * C * 5 * 8), G.flat(4)
    rc = lib.pg_loss_value_grad(S2.ptr(), ns, Sout.ptr(), None, L.LOSS_TVERSKY, N, C, HW, N, 200.0, 0.75, 0.75, vp.ptr(), vp.ld, vy.ptr(), vy.ld, 1.0,
                                vg.ptr(), vg.ld, loss.ptr(), None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    G.assert_untouched(gg, 'slice', 'loss_value_grad g')
    G.assert_untouched(Sout, 'all', 'loss_value_grad S_out'), G.assert_untouched(loss, 'all', 'loss_value_grad loss_out')
    assert torch.equal(Sout.inner(torch.float64), S.inner(torch.float64)[:N * C * 5])
    # the staged gradient
    sums = G.flat(2 * 8)
    coef, loss1 = G.flat(N * C * 2 * 4), G.flat(4)
    assert lib.pg_loss_prepare(S.ptr(), N, C, 0.75, sums.ptr(), None) == PG_OK
    assert lib.pg_loss_finalize(S.ptr(), sums.ptr(), L.LOSS_TVERSKY, N, C, HW, N, 200.0, 0.75, 0.75, coef.ptr(), loss1.ptr(), None) == PG_OK
    torch.cuda.synchronize()
    for g, name in ((sums, 'prepare local2'), (coef, 'finalize coef'), (loss1, 'finalize loss_out')):
        G.assert_untouched(g, 'all', 'loss_' + name)
    ins.add(coef, 'coef'), ins.add(S, 'S')
    vg1, gg1 = G.view(N, H, W, C, ld=C + 3, off=2)
    assert lib.pg_loss_grad(vp.ptr(), vp.ld, vy.ptr(), vy.ld, 1.0, coef.ptr(), vg1.ptr(), vg1.ld, N, HW, C, 0, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gg1, 'slice', 'loss_grad g')
    assert torch.equal(gg1.inner(), gg.inner()) and torch.equal(loss1.inner(), loss.inner())
    ins.check('loss kernels')


@pytest.mark.parametrize('dev_scalars', [False, True], ids=['adam_step', 'adam_step_dev'])
def test_adam_containment(dev_scalars):
    from tests import guard_util as G
    L, lib = _lib()
    n = 4099
    gen = torch.Generator(device='cuda').manual_seed(7)
    p0, g0 = torch.randn(n, device='cuda', generator=gen), torch.randn(n, device='cuda', generator=gen)
    p, g, m, v = G.flat_from(p0), G.flat_from(g0), G.flat_from(torch.zeros(n)), G.flat_from(torch.zeros(n))
    ins = G.Inputs()
    ins.add(g, 'g')
    bc1, sbc2 = 1.0 - 0.9, math.sqrt(1.0 - 0.999)
    if dev_scalars:
        sc = ins.add(G.flat_from(torch.tensor([1e-3 / bc1, sbc2], dtype=torch.float32)), 'scalars')
        rc = lib.pg_adam_step_dev(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 0.9, 0.999, 1e-8, sc.ptr(), None)
    else:
        rc = lib.pg_adam_step(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, 0.9, 0.999, 1e-8, bc1, sbc2, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    for b, name in ((p, 'p'), (m, 'm'), (v, 'v')):
        G.assert_untouched(b, 'all', 'adam ' + name)
    ins.check('adam')
    # first step of Adam from zero moments: p -= lr * sign-like update g / (|g| + eps)
    want = p0.double() - 1e-3 * g0.double() / (g0.double().abs() + 1e-8)
    assert (p.inner(torch.float32).double() - want).abs().max().item() < 1e-6


def test_conv_prep_batch_containment():
    """pg_conv_prep_batch: each item's u of exactly pg_conv_u_bytes, and bit-identical to what the call itself writes into u_cache."""
    from tests import guard_util as G
    L, lib = _lib()
    picked = []
    for c in sorted(conv_cases(), key=elements):
        for op in ('b2s', 's2b'):
            fam = family(kernel_name(c.geom, OPCODE[op], c.algo | io_bits(c.storage, op), ws_full(c.geom, op))[1])
            if hand_query(c, op, 'u', ws_full(c.geom, op)) and fam not in [f for f, _ in picked]:
                picked.append((fam, ConvCall(c, op, _truth(c), hand='u')))
        if len(picked) >= 4:
            break
    assert picked, 'no case has a weight cache'
    ins = G.Inputs()
    items = (L.ConvPrepItem * len(picked))()
    us = []
    for it, (fam, call) in zip(items, picked):
        if not _run_ok(call):
            pytest.fail(f'{call.what()} refused')
        u = G.flat(call.hand_bytes)
        us.append(u)
        ins.add(call.P_g, 'P')
        it.g, it.op, it.algo, it.ws_bytes, it.P, it.u = call.g, OPCODE[call.op], call.algo_io, call.full, call.P_g.ptr(), u.ptr()
    rc = lib.pg_conv_prep_batch(len(picked), items, None)
    torch.cuda.synchronize()
    assert rc == PG_OK
    for u, (fam, call) in zip(us, picked):
        G.assert_untouched(u, 'all', f'conv_prep_batch {fam}')
        assert torch.equal(u.inner(), call.hand_g.inner()), f'conv_prep_batch {fam}: differs from the call\'s own u_cache'
    ins.check('conv_prep_batch')


def test_tiles_containment():
    """pg_tiles_gather / _blend at the smallest tiled case of test_tile_kernels_non_square_and_errors (2 x 600 x 1024, 256-pixel tiles,
    overlap 0.9): tiles into a slice of ld = C + 2, the argmax map of exactly H*W int64."""
    from tests import guard_util as G
    L, lib = _lib()
    C, H, W, size, eff = 2, 600, 1024, 256, int(0.9 * 256)
    img = torch.rand(C, H, W, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9))
    ny, nx = lib.pg_tiles_count(H, size, eff), lib.pg_tiles_count(W, size, eff)
    assert (ny, nx) == (3, 5)
    ins = G.Inputs()
    gi = ins.add(G.flat_from(img), 'image')
    vt, gt = G.view(ny * nx, size, size, C, ld=C + 2, off=1)
    assert lib.pg_tiles_gather(gi.ptr(), C, H, W, size, eff, vt.ptr(), vt.ld, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gt, 'slice', 'tiles_gather')
    tiles = G.read_nchw(vt).float()
    for k in (0, ny * nx - 1):
        y0 = (k // nx) * eff - max((k // nx) * eff + size - H, 0)
        x0 = (k % nx) * eff - max((k % nx) * eff + size - W, 0)
        assert torch.equal(tiles[k], img[:, y0:y0 + size, x0:x0 + size])
    ins.add(gt, 'tiles')
    arg = G.flat(H * W * 8)
    assert lib.pg_tiles_blend(vt.ptr(), vt.ld, C, size, eff, H, W, 0.0, None, arg.ptr(), None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(arg, 'all', 'tiles_blend argmax')
    assert torch.equal(arg.inner(torch.int64).view(H, W), img.argmax(0))
    mask = G.flat(C * H * W * 8)
    assert lib.pg_tiles_blend(vt.ptr(), vt.ld, C, size, eff, H, W, 0.0, mask.ptr(), None, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(mask, 'all', 'tiles_blend mask')
    ins.check('tiles')


# ---- the data movers are exact: containment and bitwise values ---------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (2, 8, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_layout_kernels_bitwise(shape):
    from tests import guard_util as G
    L, lib = _lib()
    N, C, H, W = shape
    x = torch.randn(shape, device='cuda')
    ins = G.Inputs()
    src = ins.add(G.flat_from(x), 'nchw')
    v, g = G.view(N, H, W, C, ld=C + 4, off=4 if C % 4 == 0 else 2)
    assert lib.pg_nchw_to_nhwc(src.ptr(), v.ptr(), v.ld, N, C, H, W, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(g, 'slice', 'nchw_to_nhwc')
    assert torch.equal(G.read_nchw(v).float(), x)
    ins.add(g, 'nhwc')
    dst = G.flat(x.numel() * 4)
    assert lib.pg_nhwc_to_nchw(v.ptr(), v.ld, dst.ptr(), N, C, H, W, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(dst, 'all', 'nhwc_to_nchw')
    assert torch.equal(dst.inner(torch.float32).view(shape), x)
    ins.check('layout')


def test_copy_fill_u8_onehot_bitwise():
    from tests import guard_util as G
    L, lib = _lib()
    N, H, W = 2, 5, 7
    npix = N * H * W
    x = torch.randn(N, 3, H, W, device='cuda')
    ins = G.Inputs()
    vs, gs = G.view_from(x, ld=5, off=1)
    ins.add(gs, 'src')
    vd, gd = G.view(N, H, W, 3, ld=8, off=2)
    assert lib.pg_copy_channels(vs.ptr(), vs.ld, vd.ptr(), vd.ld, npix, 3, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gd, 'slice', 'copy_channels')
    assert torch.equal(G.read_nchw(vd).float(), x)
    for n in (1, 4099):
        f = G.flat(n * 4)
        assert lib.pg_fill(f.ptr(), n, 1.5, None) == PG_OK
        torch.cuda.synchronize()
        G.assert_untouched(f, 'all', f'fill n={n}')
        assert bool((f.inner(torch.float32) == 1.5).all().item())
    u8 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
    gu = ins.add(G.flat_from(u8), 'u8')
    vf, gf = G.view(N, H, W, 3, ld=8, off=2)
    assert lib.pg_u8_to_f32(gu.ptr(), vf.ptr(), vf.ld, npix, 3, 255.0, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gf, 'slice', 'u8_to_f32')
    # (the reference divides on the CPU: torch's GPU kernel multiplies by the reciprocal of a scalar divisor, the library divides)
    assert torch.equal(G.read_nchw(vf).float().cpu(), (u8.cpu().float() / 255.0).permute(0, 3, 1, 2))
    lab = torch.randint(0, 6, (N, H, W), dtype=torch.uint8, device='cuda')
    lab[0, 0, :3] = 255
    gl = ins.add(G.flat_from(lab), 'labels')
    labels = [0, 2, 5]
    arr = (ctypes.c_int * 3)(*labels)
    vh, gh = G.view(N, H, W, 3, ld=8, off=5)
    assert lib.pg_labels_to_onehot(gl.ptr(), vh.ptr(), vh.ld, npix, arr, 3, 1, None) == PG_OK
    torch.cuda.synchronize()
    G.assert_untouched(gh, 'slice', 'labels_to_onehot')
    want = torch.stack([((lab + 1) == v).float() for v in labels], 1)          # (uint8 arithmetic: 255 + 1 -> 0)
    assert torch.equal(G.read_nchw(vh).float(), want)
    ins.check('copy / u8 / onehot')


def test_pad_channel_writers_zero_their_pads():
    """pg_pad8_bf16 and pg_din_fill write whole pixels: the header documents that their pad channels receive zeros.  Exactly that, and
    nothing beyond ld."""
    from tests import guard_util as G
    L, lib = _lib()
    N, H, W = 2, 5, 7
    npix = N * H * W
    ins = G.Inputs()
    for C in (1, 3, 5, 8):
        x = torch.randn(N, C, H, W, device='cuda')
        vs, gs = G.view_from(x, ld=C + 2, off=1)
        ins.add(gs, 'src')
        vd, gd = G.view(N, H, W, C, ld=8, off=0, bf=True)
        assert lib.pg_pad8_bf16(vs.ptr(), vs.ld, vd.ptr(), npix, C, None) == PG_OK
        torch.cuda.synchronize()
        G.assert_untouched(gd, 'all', f'pad8_bf16 C={C}')          # every channel of the 8-channel pixels, nothing around them
        px = gd.inner(torch.bfloat16).view(N, H, W, 8)
        assert torch.equal(px[..., :C].permute(0, 3, 1, 2), x.bfloat16()) and bool((px[..., C:] == 0).all().item()), C
    for Cx, Cy, ld in ((3, 1, 4), (3, 1, 8), (3, 4, 8), (1, 2, 5)):
        x, y = torch.randn(N, Cx, H, W, device='cuda'), torch.randn(N, Cy, H, W, device='cuda')
        gx, gy = ins.add(G.flat_from(x), 'x'), ins.add(G.flat_from(y), 'y')
        real, fake = G.flat(npix * ld * 4), G.flat(npix * ld * 4)
        assert lib.pg_din_fill(gx.ptr(), gy.ptr(), real.ptr(), fake.ptr(), ld, N, Cx, Cy, H, W, None) == PG_OK
        torch.cuda.synchronize()
        G.assert_untouched(real, 'all', 'din_fill real'), G.assert_untouched(fake, 'all', 'din_fill fake')
        r, f = real.inner(torch.float32).view(N, H, W, ld), fake.inner(torch.float32).view(N, H, W, ld)
        xh, yh = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)
        assert torch.equal(r[..., :Cx], xh) and torch.equal(r[..., Cx:Cx + Cy], yh) and bool((r[..., Cx + Cy:] == 0).all().item()), (Cx, Cy, ld)
        assert torch.equal(f[..., :Cx], xh) and bool((f[..., Cx:] == 0).all().item()), (Cx, Cy, ld)
    ins.check('pad8 / din_fill')
