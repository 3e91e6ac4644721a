"""Large-view addressing tests (tests/test_bigview_cpu.py, tests/test_bigview_gpu.py): strides, arena and case lists.

Every kernel of the project addresses a [pixels][C] view through a pixel stride `ld`.  The fast conv kernels do it with 32-bit byte
offsets, in-band sentinels and `int` buffer-descriptor sizes, and therefore only below pg_conv_max_tensor_bytes() (L = 1.5 GiB); all
the others form `pixel * ld` products that must widen to 64 bits.  The device here puts real byte offsets beyond L, 2^31 and 2^32 at
microsecond cost: a small geometry (tens to thousands of pixels) with a giant `ld`, inside memory the test owns.

Arena.  One device allocation per test module, NaN-filled before each case.  The view starts APRON = 2^31 bytes into it, so an offset
taken as a signed 32-bit number still lands in owned memory.  Views are written and read with plain torch strided indexing
(`arena[...].view(P, ld)[:, :C]`), never with the layout kernels, which are themselves under test.  One operand of a call is giant,
the others compact.

Stride tiers (extent = ((P - 1) ld + C) elem bytes, the C side's tensor_bytes):
  B  the largest admissible ld with extent <  L        A  the smallest admissible ld with extent >= L
  S  at least the last quarter of the pixels start at byte offsets >= 2^31        W  ... at >= 2^32
ld % 4 == 0 (fp32) / ld % 8 == 0 (bf16) and a 16-byte-aligned base, so that alignment never changes the kernel choice.

Admissible strides (the sensitivity argument).  For every element (p, c) of the view and every w in {+-2^31, +-2^32}, the address
byte(p, c) + w lies in the apron, in an inter-pixel gap or outside [0, extent): never inside the C channels of a pixel of the view.
A read that goes wrong by a 32-bit truncation or sign error then fetches NaN (or 0 from a range-checked buffer load), a write lands
in NaN-filled memory the test owns -- and the count of non-NaN elements of the arena after the call gives it away.

Not in scope: views beyond 2^31 ELEMENTS (more than 8 GiB of fp32).  They would need 16 GiB or more of owned surroundings and no
supported configuration produces one.  For bf16 tensors tier W (2^32 bytes = 2^31 elements) is exactly that and is left out."""
import math

import numpy as np
import torch

from patchgan_amd import _lib as L
from tests import exact_util as X

GIB = 1 << 30
APRON = 1 << 31
WRAPS = (-(1 << 32), -(1 << 31), 1 << 31, 1 << 32)
TIERS = ('B', 'A', 'S', 'W')
TIER_START = {'S': 1 << 31, 'W': 1 << 32}       # byte offset the last quarter of the pixels must reach
MAX_ARENA = 8 * GIB
MAX_ARENA_BAS = 5 * GIB                         # tiers B, A and S always run


def limit():
    """pg_conv_max_tensor_bytes(): host-only."""
    return int(L.load().pg_conv_max_tensor_bytes())


def extent(P, ld, C, elem):
    """Bytes the view spans by the C side's rule (conv_gemm.hip tensor_bytes)."""
    return ((P - 1) * ld + C) * elem


def quarter_start(P):
    """Index of the first pixel of the last quarter (at least a quarter of the pixels: P - ceil(P / 4))."""
    return P - (P + 3) // 4


def admissible(P, ld, C, elem):
    """The property of the module docstring, in closed form: byte(p, c) + w = ((p + k) ld + r + c) elem with k = floor(w / elem / ld)
    and r = (w / elem) mod ld, the same for every p.  The C channels of pixel p shifted by w meet those of pixel p + k iff r < C, those
    of pixel p + k + 1 iff r + C > ld; such a pixel exists for some p iff |k| < P (|k + 1| < P)."""
    if ld < C:
        return False
    for w in WRAPS:
        k, r = divmod(w // elem, ld)
        if (r < C and abs(k) < P) or (r + C > ld and abs(k + 1) < P):
            return False
    return True


def admissible_literal(P, ld, C, elem):
    """The same property element by element, as the issue states it (the CPU test holds `admissible` to it)."""
    addr = (np.arange(P, dtype=np.int64)[:, None] * ld + np.arange(C, dtype=np.int64)[None, :]) * elem
    ext = extent(P, ld, C, elem)
    for w in WRAPS:
        a = addr + w
        inside = (a >= 0) & (a < ext)
        if bool((inside & ((a // elem) % ld < C)).any()):
            return False
    return True


def choose_ld(tier, P, C, elem, lim=None):
    """The stride of one tier for a [P][C] view of `elem`-byte elements; steps by 8 until the stride is admissible."""
    lim = limit() if lim is None else lim
    g = 8 if elem == 2 else 4
    assert tier in TIERS and P >= 4 and lim % elem == 0
    if tier == 'B':
        ld = ((lim - elem) // elem - C) // (P - 1) // g * g
        assert extent(P, ld, C, elem) < lim <= extent(P, ld + g, C, elem)
        step = -8
    elif tier == 'A':
        ld = -(-(lim // elem - C) // (P - 1))
        ld = -(-ld // g) * g
        assert extent(P, ld - g, C, elem) < lim <= extent(P, ld, C, elem)
        step = 8
    else:
        p0 = quarter_start(P)
        ld = -(-TIER_START[tier] // (elem * p0))
        ld = -(-ld // g) * g
        step = 8
    while not admissible(P, ld, C, elem):
        ld += step
    assert ld >= max(C, g) and ld % g == 0 and ld < 2 ** 31
    return ld


def in_tier(tier, P, ld, C, elem, lim):
    """Tier membership, straight from the definitions."""
    if tier == 'B':
        return extent(P, ld, C, elem) < lim
    if tier == 'A':
        return extent(P, ld, C, elem) >= lim
    return quarter_start(P) * ld * elem >= TIER_START[tier] and P - quarter_start(P) >= P / 4


def region_bytes(P, ld, elem, apron=APRON):
    """Arena bytes one view needs: the apron and P whole pixel strides (`arena[...].view(P, ld)`)."""
    return apron + P * ld * elem


def tiers_of(elem):
    return TIERS if elem == 4 else TIERS[:3]        # (bf16: tier W is 2^31 elements, out of scope)


def arena_need(P, C, elem, tiers=None, lim=None):
    return max(region_bytes(P, choose_ld(t, P, C, elem, lim), elem) for t in (tiers or tiers_of(elem)))


class Arena:
    """The owned memory: `nbytes` of fp32 on `device`, a view's base `apron` bytes in.  Filled through its bf16 alias, so that both
    the fp32 and the bf16 reading of every word are NaN (0x7FC07FC0)."""

    def __init__(self, nbytes, device, apron=APRON):
        assert nbytes % 16 == 0 and apron % 16 == 0
        self.t = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        self.apron, self.nbytes = apron, nbytes
        assert self.t.data_ptr() % 16 == 0

    def typed(self, bf):
        return self.t.view(torch.bfloat16) if bf else self.t

    def fill(self, nbytes=None):
        nbytes = self.nbytes if nbytes is None else nbytes
        assert nbytes <= self.nbytes
        self.t.view(torch.bfloat16)[:nbytes // 2].fill_(float('nan'))

    def region(self, P, ld, bf):
        elem = 2 if bf else 4
        need = region_bytes(P, ld, elem, self.apron)
        assert need <= self.nbytes, (need, self.nbytes)
        return need

    def pixels(self, P, ld, C, bf=False):
        """The [P][C] torch view of the giant operand."""
        off = self.apron // (2 if bf else 4)
        self.region(P, ld, bf)
        return self.typed(bf)[off:off + P * ld].view(P, ld)[:, :C]

    def view(self, N, H, W, C, ld, bf=False):
        """The same memory as an engine View."""
        from patchgan_amd import engine as E
        self.region(N * H * W, ld, bf)
        v = E.View(self.typed(bf), self.apron // (2 if bf else 4), ld, N, H, W, C, bf)
        assert v.ptr() % 16 == 0
        return v

    def count(self, nbytes, bf=False):
        """Non-NaN elements of the first `nbytes` (apron, view and gaps), in elements of the view's type."""
        t = self.typed(bf)[:nbytes // (2 if bf else 4)]
        step, n = 1 << 28, 0
        for i in range(0, t.numel(), step):
            c = t[i:i + step]
            n += int((c == c).sum())
        return n


def compact_ld(C, bf=False):
    g = 8 if bf else 4
    return -(-C // g) * g


def to_pixels(x):
    """NCHW -> [N H W][C] (torch)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def from_pixels(p, N, H, W):
    """[N H W][C] -> NCHW, contiguous (torch)."""
    return p.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ---- Part 1: the conv case lists ------------------------------------------------------------------------------------------------------
# kernel symbol (ConvOp.describe) -> family.  A pair "a+b" is the family of its second kernel where that names a row-GEMM path.
HEADS = {
    'k_big2small_direct': 'direct', 'k_small2big_direct': 'direct', 'k_wgrad_direct': 'direct',
    'k_big2small': 'generic', 'k_small2big': 'generic', 'k_wgrad': 'generic',
    'k_b2s_fast': 'fast', 'k_s2b_fast': 'fast', 'k_wgrad_fast': 'fast',
    'k_b2s_bf16': 'bf16 staged', 'k_s2b_bf16': 'bf16 staged', 'k_wgrad_bf16': 'bf16 staged',
    'k_b2s_tapk': 'tapk', 'k_b2s_tapkp': 'tapkp', 'k_s2b_tapnf': 'tapnf', 'k_s2b_ca1': 'ca1', 'k_s2b_ca1_s1': 'ca1_s1',
    'k_wgrad_tapn': 'wgrad_tapn', 'k_wgrad_tapnp': 'wgrad_tapnp',
    'k_wino_bgemm_s3': 'polyphase s3', 'k_wino_bgemm_s3_mz': 'polyphase s3', 'k_wino_bgemm': 'polyphase fp32', 'k_wino_bgemm_mz': 'polyphase fp32',
    'k_wino_wgrad_gemm_s3': 'polyphase wgrad s3', 'k_wino_wgrad_gemm': 'polyphase wgrad fp32',
    'k_conv_bf16x': 'bf16x', 'k_conv_bf16r': 'bf16r', 'k_wgrad_bf16x': 'wgrad_bf16x',
}
# family -> the ops it has
FAMILY_OPS = {
    'direct': (0, 1, 2), 'generic': (0, 1, 2), 'fast': (0, 1, 2), 'bf16 staged': (0, 1, 2), 'col2im': (1,), 'gather': (0,), 'tapk': (0,),
    'tapkp': (0,), 'tapnf': (1,), 'ca1': (1,), 'ca1_s1': (1,), 'wgrad_tapn': (2,), 'wgrad_tapnp': (2,), 'polyphase s3': (0, 1),
    'polyphase fp32': (0, 1), 'polyphase wgrad s3': (2,), 'polyphase wgrad fp32': (2,),
}
GENERIC = {0: 'k_big2small<1,1,4,1>', 1: 'k_small2big<1,1,4,1>', 2: 'k_wgrad<1,1,4,1>'}      # the 'gemm' budget class of tiers A, S, W


def family_of(sym):
    if sym.endswith('+k_col2im_small2big'):
        return 'col2im'
    if sym.endswith('+k_gather_big2small'):
        return 'gather'
    return HEADS[sym.split('<')[0]]


def pixels_of(geom):
    """(pixels of `big`, pixels of `small`)."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = X.dims(geom)
    return N * Hb * Wb, N * Hs * Ws


def operand_shapes(geom, op):
    """The views of one op as (role, P, C) -- the inputs first, then the output (op 2 writes packed weights: no view)."""
    N, Hb, Wb, Ca, Cb, s = geom
    pb, ps = pixels_of(geom)
    big, small = ('big', pb, Cb), ('small', ps, Ca)
    return {0: ([big], small), 1: ([small], big), 2: ([small, big], None)}[op]


def case_fits(geom, op, elem=4, lim=None):
    """Every view of the op has >= 4 pixels and a tier-W (bf16: tier-S) region within the arena bound."""
    ins, out = operand_shapes(geom, op)
    return all(P >= 4 and arena_need(P, C, elem, lim=lim) <= MAX_ARENA and arena_need(P, C, elem, TIERS[:3], lim) <= MAX_ARENA_BAS
               for _, P, C in ins + ([out] if out else []))


def exact_candidates():
    """(geometry, algo bits) of every fp32 launch group of tests/test_exact_gpu.py: GEOMS under the four algos, the fuzz list of
    seed 0, WINO2_GEOMS, WINO2W_GEOMS and BWD_BIG_GEOM in both GEMM forms."""
    from tests.test_exact_gpu import all_fp32_cases
    seen, out = set(), []
    for c in all_fp32_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


class ConvCase:
    def __init__(self, family, op, geom, algo, sym, split, klass='exact'):
        self.family, self.op, self.geom, self.algo, self.sym, self.split, self.klass = family, op, geom, algo, sym, split, klass

    @property
    def id(self):
        return f'{self.family}-op{self.op}'

    def __repr__(self):
        return f'{self.family} op {self.op} {self.geom} algo {self.algo:#x} {self.sym} split {self.split}'


_EXACT_CASES = None


def exact_cases(lim=None):
    """For each family and op: the candidate with the fewest pixels (big + small) that ConvOp.describe puts on the family."""
    global _EXACT_CASES
    if _EXACT_CASES is None:
        from patchgan_amd import engine as E
        best = {}
        for geom, algo in exact_candidates():
            cop = E.ConvOp(*geom, algo)
            for op in range(3):
                sym, split = cop.describe(op)
                key = (family_of(sym), op)
                pix = sum(pixels_of(geom))
                if (key not in best or pix < best[key][0]) and case_fits(geom, op, lim=lim):
                    best[key] = (pix, ConvCase(key[0], op, geom, algo, sym, split))
        _EXACT_CASES = [best[(f, op)][1] for f in FAMILY_OPS for op in FAMILY_OPS[f] if (f, op) in best]
    return _EXACT_CASES


def exact_case(family, op):
    for c in exact_cases():
        if (c.family, c.op) == (family, op):
            return c
    raise AssertionError(f'no case list entry reaches family {family!r} with op {op}: the planner moved it')


HANDOVER = [('polyphase s3', 0), ('polyphase s3', 1), ('polyphase fp32', 0), ('tapkp', 0)]      # (family, op) of the hand-over test


def handover_case(family, op):
    """The fewest-pixel candidate on `family` whose kernel can emit InstanceNorm partial sums (pg_conv_stats_chunks > 0: the
    image-facing persistent kernel does so under PG_ALGO_AUTO only)."""
    import ctypes
    from patchgan_amd import engine as E
    best = None
    for geom, algo in exact_candidates():
        cop = E.ConvOp(*geom, algo)
        sym, split = cop.describe(op)
        if family_of(sym) != family or not case_fits(geom, op):
            continue
        if int(L.load().pg_conv_stats_chunks(ctypes.byref(cop.g), op, algo, cop.ws_arg)) <= 0:
            continue
        if best is None or sum(pixels_of(geom)) < sum(pixels_of(best.geom)):
            best = ConvCase(family, op, geom, algo, sym, split)
    assert best is not None, f'no case list entry on {family!r} op {op} emits partial sums'
    return best


# stride-1 Winograd: (name, geometry, tuning bits, op, symbol) from tests/test_wino1_gpu.py (FWD_CASES / WGRAD_CASES: G64 is the
# smallest geometry of both lists; the dy tile edge 3 needs the 47 x 48 one).  F(2x2,4x4), the row-fused F(3x3,4x4) pair in both GEMM
# forms, F(4x4,2x2) and F(4x4,3x3).
def wino1_cases():
    from tests import test_wino1_gpu as T
    out = []
    for name, bits, want in (('wino1 F2', T.F2, T.K_F2_64), ('wino1 F3 row-fused s3', T.F3, T.K_ROW_S3), ('wino1 F3 row-fused fp32', T.F3 | T.S3_OFF, T.K_ROW)):
        for op in (0, 1):
            assert any(f[0] == bits and f[1] and f[2] == want for f in T.FWD_CASES[(T.G64, op)]), (name, op)
            out.append(ConvCase(name, op, T.G64, L.ALGO_AUTO | bits, want, 1, 'wino1'))
    for geom, r in ((T.G64, 2), ((4, 47, 48, 64, 64, 1), 3)):
        assert T.WGRAD_CASES[geom] == r
        out.append(ConvCase(f'wino1 wgrad F(4x4,{r}x{r}) s3', 2, geom, L.ALGO_AUTO, T.K_W64_S3, None, 'wino1'))
    out.append(ConvCase('wino1 wgrad F(4x4,2x2) fp32', 2, T.G64, L.ALGO_AUTO | T.S3_OFF, T.K_W64, None, 'wino1'))
    return out


def conv_cases():
    return exact_cases() + wino1_cases()


# bf16 tensors (PG_IO_*): (name, geometry, algo bits, op, io bits, symbol prefix).  Geometries from BF16_GEOMS / WINDOW_GEOMS of
# tests/test_exact_gpu.py and, for the one-channel kernel, GEOMS; chosen in bf16_cases() as the fewest-pixel one on the family.
def bf16_cases():
    from patchgan_amd import engine as E
    from tests.test_exact_gpu import BF16_GEOMS, WINDOW_GEOMS
    from tests.test_kernels_gpu import GEOMS
    want = [('bf16x flat', BF16_GEOMS, L.ALGO_BF16 | L.TUNE_BF16X_FLAT, (0, 1), L.IO_MASK, 'k_conv_bf16x<'),
            ('bf16x ring', BF16_GEOMS, L.ALGO_BF16 | L.TUNE_BF16X_RING, (0, 1), L.IO_MASK, 'k_conv_bf16x<'),
            ('bf16r', WINDOW_GEOMS, L.ALGO_BF16, (0, 1), L.IO_MASK, 'k_conv_bf16r<'),
            ('wgrad_bf16x', BF16_GEOMS, L.ALGO_BF16, (2,), L.IO_MASK, 'k_wgrad_bf16x<'),
            ('ca1 bf16 big', GEOMS, L.ALGO_BF16, (1,), L.IO_BIG_BF16, 'k_s2b_ca1')]
    out = []
    for name, geoms, algo, ops, io, prefix in want:
        for op in ops:
            best = None
            for geom in geoms:
                N, Hb, Wb, Ca, Cb, s = geom
                if Cb <= 8 and name != 'ca1 bf16 big':
                    continue            # (8-channel pixels have a fixed ld == 8: the many-pixel case)
                sym, split = E.ConvOp(*geom, algo).describe(op, io)
                if '+' in sym or not sym.startswith(prefix) or not case_fits(geom, op, 2):
                    continue
                if best is None or sum(pixels_of(geom)) < sum(pixels_of(best.geom)):
                    best = ConvCase(name, op, geom, algo, sym, split, 'bf16')
                    best.io = io
            assert best is not None, f'no bf16 case list entry reaches {name} with op {op}'
            out.append(best)
    return out


# ---- Part 2: [P][C] views of the norm, activation, BatchNorm, loss, layout, metrics, diffaug and tile kernels --------------------------
# name -> (N, H, W, C, element bytes) of the operand that is made giant (tiers S and W; bf16: S), for the CPU admissibility check
PART2_VIEWS = {}


def part2_view(name, N, H, W, C, elem=4):
    PART2_VIEWS[name] = (N, H, W, C, elem)
    return N, H, W, C


def all_views():
    """(what, P, C, elem, tiers) of every giant view of both parts: the CPU test checks each stride."""
    out = []
    from tests.test_exact_gpu import BWD_BIG_GEOM
    extra = [handover_case(f, op) for f, op in HANDOVER] + [ConvCase('bwd_big', 0, BWD_BIG_GEOM, 0, None, None)]
    for c in conv_cases() + extra:
        ins, o = operand_shapes(c.geom, c.op)
        for role, P, C in ins + ([o] if o else []):
            out.append((f'{c.id} {role}', P, C, 4, TIERS))
    for c in bf16_cases():
        ins, o = operand_shapes(c.geom, c.op)
        for role, P, C in ins + ([o] if o else []):
            bf = (role == 'big' and c.io & L.IO_BIG_BF16) or (role == 'small' and c.io & L.IO_SMALL_BF16)
            out.append((f'{c.id} {role}', P, C, 2 if bf else 4, ('B', 'A', 'S')))
    for name, (N, H, W, C, elem) in PART2_VIEWS.items():
        out.append((name, N * H * W, C, elem, ('S', 'W') if elem == 4 else ('S',)))
    return out
