"""The checker of the fused optimisation step (include/odtk_hip.h: odtk_optim_sgd_step, odtk_optim_grad_norm): the definition in
numpy, one float32 operation per rounding, independent of odtk/optim.py.

    skipped -- nothing changes -- when found_inf != 0 or (clipping) the norm is not finite; otherwise per element
    g = grad;  g = g / grad_scale;  g = g * coef;  g = g + wd * p (wd != 0)
    buf = first ? g : (momentum * buf) + g;   p = p - (lr * buf);   e = e + one_minus_decay * (p - e)

    norm = float32(sqrt(sum of double(g') * double(g'))), g' = g / grad_scale in float32: the squares are exact in double, the
           sum here is math.fsum's, the correctly rounded one
    coef = min(1, max_norm / (norm + 1e-6)) in float32; NaN stays NaN
"""
import math

import numpy as np

F = np.float32


def unscaled(grad, grad_scale):
    g = np.asarray(grad, dtype=F)
    return g if grad_scale is None else (g / F(grad_scale)).astype(F)


def exact_norm(grads, grad_scale=None):
    """sqrt of the correctly rounded sum of the squares of every unscaled gradient element, as a Python float (double)."""
    squares = []
    for g in grads:
        u = unscaled(g, grad_scale).astype(np.float64).ravel()
        squares.extend((u * u).tolist())                            # exact: a float32 squared has 48 significant bits
    total = math.fsum(squares) if all(math.isfinite(s) for s in squares) else float(np.sum(np.asarray(squares)))
    return math.sqrt(total) if total == total else float('nan')


def grad_norm(grads, grad_scale=None):
    with np.errstate(over='ignore'):
        return F(exact_norm(grads, grad_scale))


def clip_coef(norm, max_norm):
    with np.errstate(all='ignore'):
        c = F(max_norm) / (F(norm) + F(1e-6))
    return c if c != c else min(c, F(1.0))


def ulps_apart(a, b):
    """Distance of two finite float32 values of one sign in units in the last place."""
    ia, ib = (int(np.asarray(v, dtype=F).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def sgd_step(param, grad, momentum_buffer, ema, lr, momentum, weight_decay, first, one_minus_decay=0.0, grad_scale=None,
             coef=None, skip=False):
    """One step of one tensor -> (param, momentum_buffer, ema), new arrays; `ema` may be None; `momentum_buffer` is not read when
    `first`.  `skip`: the arrays come back as they are."""
    p = np.asarray(param, dtype=F)
    if skip:
        return p.copy(), None if momentum_buffer is None else np.asarray(momentum_buffer, dtype=F).copy(), None if ema is None else ema.copy()
    with np.errstate(all='ignore'):
        g = unscaled(grad, grad_scale)
        if coef is not None:
            g = (g * F(coef)).astype(F)
        if weight_decay != 0:
            g = (g + (F(weight_decay) * p).astype(F)).astype(F)
        buf = g.copy() if first else ((F(momentum) * np.asarray(momentum_buffer, dtype=F)).astype(F) + g).astype(F)
        p = (p - (F(lr) * buf).astype(F)).astype(F)
        e = None
        if ema is not None:
            e = np.asarray(ema, dtype=F)
            e = (e + (F(one_minus_decay) * (p - e).astype(F)).astype(F)).astype(F)
    return p, buf, e


def step_all(params, grads, buffers, emas, lr, momentum, weight_decay, one_minus_decay=0.0, grad_scale=None, max_norm=None,
             found_inf=False, norm=None):
    """One step of a whole tensor list, the norm included -> (params, buffers, emas, norm, coef).  buffers[i] None: the tensor's
    first step; a skipped first step leaves zeros (what FusedSGD allocates).  `norm`: the float32 norm to clip with instead of
    this module's own (a summation in another order may round the last bit the other way: the caller checks that distance)."""
    coef = None
    skip = bool(found_inf)
    if max_norm is not None:
        norm = grad_norm(grads, grad_scale) if norm is None else F(norm)
        coef = clip_coef(norm, max_norm)
        skip = skip or not np.isfinite(norm)
    out = ([], [], [])
    for p, g, b, e in zip(params, grads, buffers, emas):
        if skip and b is None:
            b = np.zeros_like(np.asarray(p, dtype=F))
        new = sgd_step(p, g, b, e, lr, momentum, weight_decay, b is None, one_minus_decay, grad_scale, coef, skip)
        for k in range(3):
            out[k].append(new[k])
    return out[0], out[1], out[2], norm, coef


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_values(a, b):
    """same_bits, but two NaNs count as equal whatever their sign and payload (those differ between processors)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def decay_at(decay, t):
    return min(decay, (1.0 + t) / (10.0 + t))
