#!/usr/bin/env python
"""What the fused optimisation step costs on the device (include/odtk_hip.h: odtk_optim_grad_norm, odtk_optim_sgd_step;
csrc/optim.hpp) next to the same work done by torch on the same commit: RN50FPN's real parameter shapes (frozen parameters left out,
as in training), channels_last, random gradients, no model forward -- the optimizer's passes alone, back to back.

  fused  = norm (one launch per 64 tensors + the finish) + step with the clip factor, the unscale, weight decay, momentum and the EMA
  torch  = GradScaler's unscale (torch._amp_foreach_non_finite_check_and_unscale_) + clip_grad_norm_(foreach=True) +
           SGD(foreach=True).step() + torch._foreach_lerp_ for the EMA

The two are timed in turns, round after round, in one process (events around `--iters` back-to-back steps, after a warm-up); the
bytes are the algorithmic ones, counted from the shapes: the norm reads the gradients once; the step reads gradient, parameter,
momentum and average and writes the last three.  torch's passes are counted the same way, pass by pass (unscale: read + write the
gradients; clip: read them for the norm, read + write them for the factor; SGD with weight decay and momentum: its foreach passes;
lerp: read both, write one).  Share of peak = bytes / time / 8 TB/s (HBM; MI355X_MICROARCH.md).

  python tools/fused_step_probe.py [--iters 50] [--rounds 5]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import torch

from odtk.model import Model
from odtk.optim import FusedSGD, ModelEMA

HBM_PEAK = 8.0e12


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                   # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--backbone', default='ResNet50FPN')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a timing from anywhere else says nothing'
    torch.manual_seed(0)

    def parameters():
        model = Model(args.backbone, classes=80)
        model.initialize(None)
        model = model.cuda().to(memory_format=torch.channels_last)
        model.freeze_unused_params()
        return model, [p for p in model.parameters() if p.requires_grad]

    scale = torch.tensor(65536.0, device='cuda')
    inv_scale, found_inf, zero = scale.reciprocal(), torch.zeros((), device='cuda'), torch.zeros((), device='cuda')

    model_f, params_f = parameters()
    grads = [torch.randn_like(p) * 65536.0 for p in params_f]
    fused = FusedSGD(params_f, lr=1e-6, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    fused.bind_ema(ModelEMA(model_f, 0.9998))

    def fused_step():
        for p, g in zip(params_f, grads):
            p.grad = g
        fused.grad_scale, fused.found_inf = scale, zero
        fused.step()

    model_t, params_t = parameters()
    work = [g.clone() for g in grads]
    plain = torch.optim.SGD(params_t, lr=1e-6, momentum=0.9, weight_decay=1e-4, foreach=True)
    shadow = [p.detach().clone() for p in params_t]

    def torch_step():
        torch._foreach_copy_(work, grads)                           # (the unscale is in place: start from the scaled gradients)
        for p, g in zip(params_t, work):
            p.grad = g
        torch._amp_foreach_non_finite_check_and_unscale_(work, found_inf, inv_scale)
        torch.nn.utils.clip_grad_norm_(params_t, 35.0, foreach=True)
        plain.step()
        torch._foreach_lerp_(shadow, [p.detach() for p in params_t], 0.0002)

    def copy_only():
        torch._foreach_copy_(work, grads)

    n = sum(p.numel() for p in params_f)
    word = 4 * n
    fused_bytes = word + 7 * word                                   # norm: 1 read; step: 4 reads + 3 writes
    torch_bytes = 2 * word + 3 * word + (3 + 3 + 3) * word + 3 * word   # unscale; clip; wd add, momentum mul-add, update; lerp
    print('%s: %d tensors with a gradient, %.2f M parameters = %.1f MB per array' % (args.backbone, len(params_f), n / 1e6, word / 1e6))
    rows = {'fused norm + step + EMA': [], 'torch unscale + clip + SGD + lerp (+ gradient copy)': [], 'the gradient copy alone': []}
    for _ in range(args.rounds):
        rows['fused norm + step + EMA'].append(timed(fused_step, args.iters))
        rows['torch unscale + clip + SGD + lerp (+ gradient copy)'].append(timed(torch_step, args.iters))
        rows['the gradient copy alone'].append(timed(copy_only, args.iters))
    med = {k: statistics.median(v) for k, v in rows.items()}
    for k, v in rows.items():
        print('%-52s median %8.1f us   rounds: %s' % (k, med[k], ' '.join('%.1f' % x for x in v)))
    torch_us = med['torch unscale + clip + SGD + lerp (+ gradient copy)'] - med['the gradient copy alone']
    for name, us, nbytes in (('fused', med['fused norm + step + EMA'], fused_bytes), ('torch (copy subtracted)', torch_us, torch_bytes)):
        print('%-24s %8.1f us per step, %7.1f MB moved, %.2f TB/s = %.2f of HBM peak' % (name, us, nbytes / 1e6, nbytes / us / 1e6,
                                                                                      nbytes / (us * 1e-6) / HBM_PEAK))
    print('(times are per optimizer step between events, host enqueue included: %d launches of the library per fused step)'
          % (2 * ((len(params_f) + 63) // 64) + 1))


if __name__ == '__main__':
    main()
