"""Gradient accumulation: the float32 NumPy replay of pg_grad_accum's four modes and of a whole window, the mixed test inputs, and the
calling sequence of a window.

The kernel does per element ONE fp32 add and then ONE fp32 multiply, never fused, so numpy.float32 arithmetic in that order IS the
reference: the comparison is array_equal on the bits (NaN positions included, NaN payloads aside)."""
import numpy as np

BEGIN, ADD, CLOSE, CLOSE_ONLY = 0, 1, 2, 3          # PG_ACC_*
F32 = np.float32
NS = (1, 3, 4, 5, 1023, 1024, 4099)


def scale_of(count):
    """1 / count formed in double and rounded once: what the host hands the closing modes."""
    return F32(1.0 / count)


def replay(mode, acc, g, scale=1.0):
    """(acc', g') after one call of `mode` on float32 arrays; the operand a mode only reads is returned as it came."""
    acc, g = np.asarray(acc, dtype=F32), np.asarray(g, dtype=F32)
    with np.errstate(all='ignore'):
        if mode == BEGIN:
            return g.copy(), g
        if mode == ADD:
            return acc + g, g
        if mode == CLOSE:
            return acc, (acc + g) * F32(scale)
        if mode == CLOSE_ONLY:
            return acc, acc * F32(scale)
    raise ValueError(mode)


def window(grads, short=False):
    """The closed gradient of a window over the float32 arrays `grads`: BEGIN, ADD ..., CLOSE with fl(1 / len) -- or, short=True, every
    gradient accumulated and the window closed by CLOSE_ONLY.  -> (the accumulator as the closing call read it, the closed gradient)."""
    acc = None
    body = grads if short else grads[:-1]
    for i, g in enumerate(body):
        acc, _ = replay(BEGIN if i == 0 else ADD, acc if acc is not None else g, g)
    if short:
        return replay(CLOSE_ONLY, acc, grads[-1], scale_of(len(grads)))
    return replay(CLOSE, acc, grads[-1], scale_of(len(grads)))


def window_f64(grads):
    """The same mean in float64 (exact for dyadic inputs whose sum and scale stay representable)."""
    return sum(np.asarray(g, dtype=np.float64) for g in grads) * (1.0 / len(grads))


def same_bits(a, b):
    """array_equal on the bits, any NaN equal to any NaN (a NaN's payload is not part of the contract), -0 distinct from +0."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def mixed(n, seed):
    """n floats: normal values of mixed magnitude with denormals, +-0, an inf and a NaN planted where n has the room."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(F32)
    plant = [F32(1e-40), F32(-3e-45), F32(0.0), F32(-0.0), F32(np.inf), F32(np.nan), F32(-np.inf)]
    if n >= 64:
        # (spread over the body, its ragged end and the tail; each array of a window gets its specials at other places)
        where = rng.choice(n - 3, size=len(plant), replace=False)
        for i, v in zip(where, plant):
            x[i] = v
        x[n - 1 - (seed % 3)] = plant[seed % len(plant)]
    elif n >= 3:
        x[seed % n] = plant[seed % len(plant)]
    return x


def dyadic(n, seed):
    """n floats k / 8 with |k| <= 2^12: sums of a few of them and a scale of 1/2, 1/4 are exact in float32 and float64."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-4096, 4097, n) / 8.0).astype(F32)


def phases(k, calls, discard_after=()):
    """The phase of each of `calls` training calls at window length k through the trainer's own helper; after the calls whose 1-based
    numbers are in `discard_after` the open window is discarded (setup_optimizers(), load(), a step that raised)."""
    from patchgan_amd import engine as E
    out, done = [], 0
    for i in range(1, calls + 1):
        ph = E.accum_phase(done, k)
        out.append(ph)
        done = 0 if ph == 'close' else done + 1
        if i in discard_after:
            done = 0
    return out
