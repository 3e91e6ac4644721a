"""Operands on which the conv kernels' fp32 arithmetic is EXACT, the precondition that proves it, and a NumPy model of the
split-bf16 polyphase Winograd GEMM (tests/test_exact_cpu.py, tests/test_exact_gpu.py).

On small integers (or fixed-point values of few bits) every product and every partial sum of a convolution, in any summation
order, is representable in fp32, so a kernel's result must EQUAL the float64 convolution: any difference is a dropped, doubled
or misplaced term, not rounding.  That holds for the direct kernels, the implicit GEMMs (fp32 and bf16 MFMA, split-K), the
small-channel kernels, the column sums of the bias gradient, and the polyphase stride-2 Winograd paths, whose transform tables
(copied below from patchgan_amd/csrc/conv_wino.hip; the CPU test compares them with the source) hold only 0, +-1 and +-0.5.
It does not hold for the stride-1 Winograd paths (1/3, 1/6, 1/15 in their tables) nor for the opt-in polyphase tile with
output edge 4 (2/9)."""
import math
import re

import numpy as np
import torch

# geometry tuples are the suite's (N, Hb, Wb, Ca, Cb, stride): `big` is [N, Cb, Hb, Wb], `small` [N, Ca, Hs, Ws], W [Ca, Cb, 4, 4]
OP_B2S, OP_S2B, OP_WGRAD = 0, 1, 2
BUDGET = 2.0 ** 24          # fp32 significand

# polyphase F(3x3, 2x2) forward / data gradient and F(2x2, 3x3) weight gradient (conv_wino.hip: c_BT3, c_G3, c_A3T, c_G23, c_A2T)
BT3 = np.array([[-1, 0, 1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], np.float32)
G3 = np.array([[-1, 0], [0.5, 0.5], [0.5, -0.5], [0, 1]], np.float32)
A3T = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], np.float32)
G23 = np.array([[-1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float32)
A2T = np.array([[1, 1, 1, 0], [0, 1, -1, 1]], np.float32)
TABLES = {'c_BT3': BT3, 'c_G3': G3, 'c_A3T': A3T, 'c_G23': G23, 'c_A2T': A2T}


def _gain(t):
    """Largest sum of |entries| over a row: how much one 1-D application of the table can grow max |x|."""
    return float(np.abs(t).sum(1).max())


# read off the tables (both axes): the input transform grows values 4x, the weight transform not at all but quarters the least
# significant bit, the output transforms sum at most 9 terms; G23 grows dy 2.25x and quarters its least significant bit
GAIN_IN, GAIN_W, LSB_W, TERMS_OUT = _gain(BT3) ** 2, _gain(G3) ** 2, 0.25, int(_gain(A3T) ** 2)
GAIN_DY, LSB_DY, TERMS_OUT_W = _gain(G23) ** 2, 0.25, int(_gain(A2T) ** 2)


def source_tables(path, names=None):
    """The same tables parsed out of conv_wino.hip (names: default those of TABLES).  An entry is a literal or a quotient of two
    (`-16.f / 15`), evaluated as the compiler does: in fp32."""
    src = open(path).read()
    out = {}
    for name in (TABLES if names is None else names):
        m = re.search(r'float %s\[(\d+)\]\[(\d+)\] = (\{.*?\});' % name, src, re.S)
        vals = [np.float32(num) / np.float32(den or 1) for num, den in re.findall(r'(-?\d+\.?\d*)f?(?:\s*/\s*(\d+\.?\d*)f?)?', m.group(3))]
        out[name] = np.array(vals, np.float32).reshape(int(m.group(1)), int(m.group(2)))
    return out


def dims(geom):
    N, Hb, Wb, Ca, Cb, s = geom
    return (Hb - 2) // s + 1, (Wb - 2) // s + 1


def _gen(geom, seed):
    N, Hb, Wb, Ca, Cb, s = geom
    return torch.Generator().manual_seed(((((((seed * 31 + N) * 131 + Hb) * 131 + Wb) * 521 + Ca) * 521 + Cb) * 3 + s) & 0x7FFFFFFF)


class Operands:
    """fp32 CPU tensors of one geometry; amax / lsb: bound and least significant bit of (big, small, W), for the budget."""

    def __init__(self, geom, big, small, Wt, bias_a=None, bias_b=None, lsb=(1.0, 1.0, 1.0)):
        self.geom, self.big, self.small, self.Wt, self.bias_a, self.bias_b, self.lsb = geom, big, small, Wt, bias_a, bias_b, lsb
        self.amax = tuple(float(t.abs().max()) for t in (big, small, Wt))
        self.bias_max = max([float(b.abs().max()) for b in (bias_a, bias_b) if b is not None] or [0.0])


def exact_operands(geom, seed=0):
    """Activations: integers in [-3, 3]; weights: integers in [-2, 2]; biases: integers in [-4, 4].  All bf16-representable."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = dims(geom)
    g = _gen(geom, seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    return Operands(geom, ri(-3, 3, N, Cb, Hb, Wb), ri(-3, 3, N, Ca, Hs, Ws), ri(-2, 2, Ca, Cb, 4, 4), ri(-4, 4, Ca), ri(-4, 4, Cb))


def assert_exact_budget(geom, op, path, a_max, b_max, a_lsb=1.0, b_lsb=1.0, bias_max=0.0, terms=None, gain_dy=GAIN_DY):
    """The precondition of a zero-tolerance comparison: (worst-case |partial sum|) / (least significant bit of any term) < 2^24,
    so every partial sum in any order is an fp32 number.  A condition on the INPUTS (bounds and least significant bits of the two
    operands: a = the activations of ops 0 / 1, `small` of op 2; b = the weights, `big` of op 2), never a measurement of a result.
    path: 'gemm' (direct / implicit GEMM / small-channel kernels), 'wino2' (polyphase forward / data gradient), 'wino2w' (polyphase
    weight gradient).  terms: non-zero terms per reduction where the construction of the operands bounds them below the dense count.
    Returns the ratio (for the record the tests print)."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = dims(geom)
    assert path in ('gemm', 'wino2', 'wino2w') and op in (0, 1, 2), (path, op)
    if path == 'gemm':
        K = 16 * (Cb if op == 0 else Ca) if op < 2 else N * Hs * Ws
        worst, lsb = min(K, terms or K) * a_max * b_max + bias_max, a_lsb * b_lsb
    elif path == 'wino2':
        assert op < 2 and s == 2, (geom, op)
        K = 4 * (Cb if op == 0 else Ca)         # (op 1 reduces over Ca only: the four classes are columns there; 4 Ca bounds it)
        worst = TERMS_OUT * min(K, terms or K) * (GAIN_IN * a_max) * (GAIN_W * b_max) + bias_max
        lsb = a_lsb * b_lsb * LSB_W
    else:
        assert op == 2 and s == 2, (geom, op)
        T = N * ((Hs + 2) // 3) * ((Ws + 2) // 3)
        worst = TERMS_OUT_W * min(T, terms or T) * (gain_dy * a_max) * (GAIN_IN * b_max)
        lsb = a_lsb * LSB_DY * b_lsb
    ratio = worst / lsb
    assert ratio < BUDGET, f'not provably exact: {geom} op {op} {path}: worst partial sum {worst} / lsb {lsb} = 2^{math.log2(ratio):.2f} >= 2^24'
    return ratio


def path_of(sym, stride):
    """Budget class of a kernel symbol (ConvOp.describe); the non-dyadic Winograd kernels are refused."""
    assert not sym.startswith('k_wino_gemm'), f'{sym}: stride-1 Winograd (1/3, 1/6, 1/15 in its tables) is not exact'
    if sym.startswith('k_wino'):
        assert stride == 2, f'{sym} on a stride-1 layer: not in the exact class'
        return 'wino2w' if sym.startswith('k_wino_wgrad') else 'wino2'
    return 'gemm'


def budget_for(ops, op, sym):
    """assert_exact_budget of dense operands `ops` for opcode `op` run by kernel `sym`."""
    s = ops.geom[5]
    big, small, w = zip(ops.amax, ops.lsb)
    a, b = ((big, w), (small, w), (small, big))[op]
    return assert_exact_budget(ops.geom, op, path_of(sym, s), a[0], b[0], a[1], b[1], ops.bias_max if op < 2 else 0.0)


def to_fp32_exact(want64):
    """The float64 reference as fp32, after checking that it survives the round trip."""
    w32 = want64.float()
    assert torch.equal(w32.double(), want64), 'the float64 reference is not an fp32 tensor'
    return w32


def reference64(ops, op, act='none', bias=True):
    """float64 torch result of opcode `op` on the device the operands live on.  op 2 returns (dW [Ca, Cb, 4, 4], dbias [Ca])."""
    import torch.nn.functional as F
    N, Hb, Wb, Ca, Cb, s = ops.geom
    Hs, Ws = dims(ops.geom)
    d = lambda t: t.double() if t is not None else None
    if op == 0:
        r = F.conv2d(d(ops.big), d(ops.Wt), d(ops.bias_a) if bias else None, stride=s, padding=1)
    elif op == 1:
        opad = (Hb - ((Hs - 1) * s + 2), Wb - ((Ws - 1) * s + 2))
        r = F.conv_transpose2d(d(ops.small), d(ops.Wt), d(ops.bias_b) if bias else None, stride=s, padding=1, output_padding=opad)
        assert tuple(r.shape[2:]) == (Hb, Wb)
    else:
        return torch.nn.grad.conv2d_weight(d(ops.big), (Ca, Cb, 4, 4), d(ops.small), stride=s, padding=1), d(ops.small).sum((0, 2, 3))
    assert act in ('none', 'relu')
    return r.clamp_min(0) if act == 'relu' else r


# ---- wide-significand operands for the split-bf16 GEMMs --------------------------------------------------------------------------
# small integers live in the first bf16 piece alone.  (i, j) = bf16 pieces the two GEMM operands need: fractional bits of the
# wide values below.  Each reduction has ONE non-zero term by construction, so the budget is TERMS_OUT * GAIN_IN * |x| * |w| over
# 2^-(bits_x + bits_w + 2): 36 * 2^18 < 2^24 for all three.
WIDE = {'3,1': (16, 0), '1,3': (0, 16), '2,2': (8, 8)}


def _fixed(g, bits, *shape):
    """q * 2^-bits with 2^(bits-1) <= |q| < 2^bits (every value non-zero and `bits` wide); bits = 0: -1, 0 or 1."""
    if bits == 0:
        return torch.randint(-1, 2, shape, generator=g).float()
    q = torch.randint(2 ** (bits - 1), 2 ** bits, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return (q.double() * 2.0 ** -bits).float()


def _nonzero(g, bits, *shape):
    return _fixed(g, bits, *shape) if bits else (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def wide_conv_operands(geom, op, shape, seed=0):
    """op 0 / 1.  Activations: fixed point of WIDE[shape][0] bits.  Weights: a signed gather -- output channel co reads input channel
    (5 co + 3) % Cin through one tap that varies with co (+-1), or, for wide weights, through the four taps of one phase (same parity
    of kh and of kw: the transformed weight holds their signed sums / 4, two bits wider than any of them -- the sum of TWO 16-bit
    values still fits two round-to-nearest bf16 pieces, 8 + 1 + 8 bits, and would never reach the third).  The float64 result is a
    shifted copy (or a four-term combination) of the input; every Winograd-domain reduction has one non-zero term."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = dims(geom)
    xb, wb = WIDE[shape]
    g = _gen(geom, 7919 * (seed + 1) + op)
    big = _fixed(g, xb, N, Cb, Hb, Wb) if op == 0 else torch.zeros(N, Cb, Hb, Wb)
    small = _fixed(g, xb, N, Ca, Hs, Ws) if op == 1 else torch.zeros(N, Ca, Hs, Ws)
    cin, cout = (Cb, Ca) if op == 0 else (Ca, Cb)
    co = torch.arange(cout)
    ci = (5 * co + 3) % cin
    kh, kw = 2 * ((co >> 2) & 1) + (co & 1), 2 * ((co >> 3) & 1) + ((co >> 1) & 1)
    Wt = torch.zeros(Ca, Cb, 4, 4)
    a, b = (co, ci) if op == 0 else (ci, co)
    for dh, dw in ((0, 0), (2, 0), (0, 2), (2, 2)) if wb else ((0, 0),):
        Wt[a, b, kh ^ dh, kw ^ dw] = _nonzero(g, wb, cout)
    return Operands(geom, big, small, Wt, lsb=(2.0 ** -xb, 2.0 ** -xb, 2.0 ** -wb))


def wide_wgrad_operands(geom, shape, seed=0):
    """The transposed construction for op 2: `big` is fixed point of WIDE[shape][0] bits; channel a of `small` is non-zero in one
    sample at one pixel (a different 3x3 tile per channel; the 2x2 block at that tile's origin for wide `small`, so that the
    transformed dy holds signed sums / 4 of four values), so dW is a gather of `big` and every reduction over tiles has one non-zero
    term.  On rows / columns 0 and 1 of a tile G23 applies -1 to one value or halves to two: the transformed dy is no larger than dy
    (gain 1; the CPU test checks it)."""
    N, Hb, Wb, Ca, Cb, s = geom
    Hs, Ws = dims(geom)
    xb, wb = WIDE[shape]
    g = _gen(geom, 104729 * (seed + 1))
    big = _fixed(g, xb, N, Cb, Hb, Wb)
    small = torch.zeros(N, Ca, Hs, Ws)
    TH, TW = (Hs + 2) // 3, (Ws + 2) // 3
    a = torch.arange(Ca)
    t = (a * 37 + 11) % (TH * TW)
    y, x = 3 * (t // TW), 3 * (t % TW)
    x = torch.where(x + 1 < Ws, x, torch.zeros_like(x))      # (a one-column ragged tile has no neighbour: first tile of the row)
    y = torch.where(y + 1 < Hs, y, torch.zeros_like(y))
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)) if wb else ((0, 0),):
        small[a % N, a, y + dy, x + dx] = _nonzero(g, wb, Ca)
    return Operands(geom, big, small, torch.zeros(Ca, Cb, 4, 4), lsb=(2.0 ** -xb, 2.0 ** -wb, 1.0))


def wide_budget(ops, op):
    """The budget of a wide case on its polyphase path: one non-zero term per reduction, unit gain of the transformed one-hot dy."""
    big, small, w = zip(ops.amax, ops.lsb)
    if op == 2:
        return assert_exact_budget(ops.geom, 2, 'wino2w', small[0], big[0], small[1], big[1], terms=1, gain_dy=1.0)
    x = big if op == 0 else small
    return assert_exact_budget(ops.geom, op, 'wino2', x[0], w[0], x[1], w[1], terms=1)


# ---- the split-bf16 GEMM and the polyphase paths around it, in NumPy fp32 ------------------------------------------------------
def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def s3_split(x):
    """conv_wino.hip s3_split: a = a1 + a2 + a3, a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)."""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    r1 = x - h
    m = bf16_rne(r1)
    return h, m, bf16_rne(r1 - m)


S3_PRODUCTS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))      # (piece of a, piece of b), the order of k_wino_bgemm_s3


def s3_model(A, B, drop=None, rng=None, kc=16):
    """C[m][n] = sum_k A[m][k] B[n][k] as k_wino_bgemm_s3 / k_wino_wgrad_gemm_s3 form it: both operands split into three bf16
    pieces, the six products a_i b_j with i + j <= 4 per 16-wide K chunk, every addition rounded to fp32.  drop: one (i, j) of
    S3_PRODUCTS to leave out; rng: a random.Random that shuffles the order of chunks, products and k (else the kernel's)."""
    pa, pb = s3_split(A), s3_split(B)
    K = pa[0].shape[1]
    acc = np.zeros((pa[0].shape[0], pb[0].shape[0]), np.float32)
    chunks = list(range(0, K, kc))
    if rng:
        rng.shuffle(chunks)
    for c0 in chunks:
        prods = [p for p in S3_PRODUCTS if p != drop]
        ks = list(range(c0, min(c0 + kc, K)))
        if rng:
            rng.shuffle(prods)
            rng.shuffle(ks)
        for i, j in prods:
            for k in ks:
                if pa[i][:, k].any() and pb[j][:, k].any():
                    acc = acc + pa[i][:, k, None] * pb[j][None, :, k]      # (bf16 x bf16 is exact in fp32; the sum rounds)
    return acc


def _phase_windows(big, TH, TW):
    """V[xi][tile][ph * Cb + b] = (BT3 X_ph BT3^T)[xi] over the 4x4 windows at (3 ti, 3 tj) of X_rs[i][j] = big[2i+r-1][2j+s-1]."""
    N, Cb, Hb, Wb = big.shape
    X = np.zeros((N, 4, Cb, 3 * TH + 1, 3 * TW + 1), np.float32)
    for r in range(2):
        for s in range(2):
            for i in range(3 * TH + 1):
                for j in range(3 * TW + 1):
                    y, x = 2 * i + r - 1, 2 * j + s - 1
                    if 0 <= y < Hb and 0 <= x < Wb:
                        X[:, 2 * r + s, :, i, j] = big[:, :, y, x]
    V = np.zeros((16, N * TH * TW, 4 * Cb), np.float32)
    for n in range(N):
        for ti in range(TH):
            for tj in range(TW):
                d = X[n, :, :, 3 * ti:3 * ti + 4, 3 * tj:3 * tj + 4].reshape(4 * Cb, 4, 4)
                V[:, (n * TH + ti) * TW + tj, :] = np.einsum('ai,kij,bj->abk', BT3, d, BT3).reshape(16, -1)
    return V


def polyphase_fwd_model(big, Wt, gemm=s3_model):
    """big -> small of a stride-2 layer as the polyphase F(3x3, 2x2) path computes it (comment above c_BT3 in conv_wino.hip), fp32."""
    big, Wt = np.asarray(big, np.float32), np.asarray(Wt, np.float32)
    N, Cb, Hb, Wb = big.shape
    Ca = Wt.shape[0]
    Hs, Ws = (Hb - 2) // 2 + 1, (Wb - 2) // 2 + 1
    TH, TW = (Hs + 2) // 3, (Ws + 2) // 3
    V = _phase_windows(big, TH, TW)
    U = np.zeros((16, Ca, 4 * Cb), np.float32)
    for r in range(2):
        for s in range(2):
            U[:, :, (2 * r + s) * Cb:(2 * r + s + 1) * Cb] = np.einsum('iu,abuv,jv->ijab', G3, Wt[:, :, r::2, s::2], G3).reshape(16, Ca, Cb)
    M = np.stack([gemm(V[xi], U[xi]) for xi in range(16)]).reshape(4, 4, N, TH, TW, Ca)
    out = np.einsum('pi,ijnhwa,qj->nahpwq', A3T, M, A3T).reshape(N, Ca, 3 * TH, 3 * TW)
    return out[:, :, :Hs, :Ws]


def polyphase_wgrad_model(big, small, gemm=s3_model):
    """dW [Ca, Cb, 4, 4] of a stride-2 layer as the polyphase F(2x2, 3x3) path computes it (comment above c_G23), fp32."""
    big, small = np.asarray(big, np.float32), np.asarray(small, np.float32)
    N, Cb, Hb, Wb = big.shape
    _, Ca, Hs, Ws = small.shape
    TH, TW = (Hs + 2) // 3, (Ws + 2) // 3
    V = _phase_windows(big, TH, TW)
    dy = np.zeros((N, Ca, 3 * TH, 3 * TW), np.float32)
    dy[:, :, :Hs, :Ws] = small
    dy = dy.reshape(N, Ca, TH, 3, TW, 3)
    DY = np.einsum('iu,nahuwv,jv->ijnhwa', G23, dy, G23).reshape(16, N * TH * TW, Ca)
    S = np.stack([gemm(DY[xi].T, V[xi].T) for xi in range(16)]).reshape(4, 4, Ca, 2, 2, Cb)
    dW = np.einsum('ui,ijarsb,vj->aburvs', A2T, S, A2T)         # tap (2u + r, 2v + s)
    return dW.reshape(Ca, Cb, 4, 4), DY
