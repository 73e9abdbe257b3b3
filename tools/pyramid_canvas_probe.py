#!/usr/bin/env python
"""Premise check of the pyramid canvas ("Pyramid canvas"): do the head towers of the small pyramid levels cost less as
ONE convolution over a packed canvas than as one launch per level, and how much of their time is exposed in the step today?

    python tools/pyramid_canvas_probe.py --out profiles/pyramid_canvas_probe.txt            # both legs
    python tools/pyramid_canvas_probe.py --leg trace --name pyramid_canvas --out-dir DIR    # the kernel trace alone

Two legs, each a child process of its own under its own time limit; the second runs only if the first ended well, nothing is retried.
  trace  `rocprofv3 --kernel-trace --stats -- python bench.py --gpus 1 --steps 50 --warmup 10` (the form tools/profile_round.sh
         uses), then per timed step: the wall span of the head phase and the summed duration of the kernels that ran beside P3.
         The towers are the only part of the step that uses side streams, so "a dispatch that is not on the queue of the step's
         prefilter launch" names the kernels of the levels below P3 exactly; the head phase is taken from the first of them (the
         side streams are released by the event that also precedes P3's first tower kernel) to the start of the prefilter.
  time   `_C.conv_bias_act` on a tower layer (3x3, 256 -> 256, bias + ReLU, bf16, batch 8) over the canvas 8x256x50x121 (P4..P7)
         and over 8x256x25x72 (P5..P7), against the per-level launches each replaces, back to back on one stream: medians of 30
         groups after a warm-up.  The committed plan's library lines are loaded first, so the per-level problems run the instances
         the benchmark runs and the canvas problems take a planned sibling's instance, as they do in the engine.
"""
import argparse
import json
import os
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'retinanet-examples_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS, WARMUP = 50, 10
LEVELS = [(50, 80), (25, 40), (13, 20), (7, 10)]                       # P4..P7 of an 800 x 1280 input
PLAN = os.path.join(ROOT, 'plans', 'rn50fpn_bf16_bs8_800x1280.json')


def find_db(directory):
    for base, _, files in os.walk(directory):
        for f in files:
            if f.endswith('_results.db'):
                return os.path.join(base, f)
    return None


def analyse(db, steps, say):
    """Per timed step of a traced bench.py run: head-phase span and the kernels beside P3 (see the module docstring)."""
    con = sqlite3.connect(db)
    cur = con.cursor()
    cur.execute('select d.*, s.kernel_name from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start')
    cols = [c[0] for c in cur.description]
    rows = [dict(zip(cols, r)) for r in cur.fetchall()]
    marks = [i for i, r in enumerate(rows) if 'prefilter_scan' in r['kernel_name']]
    if len(marks) < steps + 1:
        say('trace: only %d prefilter launches, wanted more than %d' % (len(marks), steps))
        return False
    lane = next((c for c in ('stream_id', 'queue_id') if c in cols and len({r[c] for r in rows[marks[-steps - 1]:marks[-1]]}) > 1), None)
    if lane is None:
        say('trace: the dispatches of a step do not differ in stream_id or queue_id: no side streams visible')
        return False
    spans, sides, counts, steps_ns, sums = [], [], [], [], []
    detail = None
    for k in range(steps):
        lo, hi = marks[-steps - 1 + k], marks[-steps + k]
        window = rows[lo + 1:hi]
        end = rows[hi]
        side = [r for r in window if r[lane] != end[lane]]
        if not side:
            say('trace: step %d has no side-stream dispatch' % k)
            return False
        begin = min(r['start'] for r in side)
        spans.append((end['start'] - begin) / 1e3)
        sides.append(sum(r['end'] - r['start'] for r in side) / 1e3)
        counts.append(len(side))
        steps_ns.append((end['start'] - rows[lo]['start']) / 1e3)
        in_phase = [r for r in window if r['start'] >= begin]
        sums.append(sum(r['end'] - r['start'] for r in in_phase) / 1e3)
        if k == steps - 1:
            detail = (begin, in_phase, end[lane])

    def med(v):
        return sorted(v)[len(v) // 2]
    say('trace: lanes told apart by %s; %d timed steps' % (lane, steps))
    say('  step (prefilter to prefilter)      median %9.1f us   min %9.1f   max %9.1f' % (med(steps_ns), min(steps_ns), max(steps_ns)))
    say('  head-phase wall span               median %9.1f us   min %9.1f   max %9.1f' % (med(spans), min(spans), max(spans)))
    say('  kernel time inside the head phase  median %9.1f us' % med(sums))
    say('  kernels beside P3 (side streams)   median %9.1f us summed, %d launches per step' % (med(sides), med(counts)))
    say('  last step, side-stream kernels by name:')
    begin, in_phase, main_lane = detail
    by = {}
    for r in in_phase:
        if r[lane] != main_lane:
            key = (r['kernel_name'][:100], tuple(r.get(c) for c in ('grid_size_x', 'grid_size_y', 'grid_size_z') if c in r))
            e = by.setdefault(key, [0, 0.0])
            e[0] += 1
            e[1] += (r['end'] - r['start']) / 1e3
    for (name, grid), (n, us) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        say('    %3d x %8.1f us  grid %-18s %s' % (n, us, 'x'.join(str(g) for g in grid), name))
    return True


def leg_trace(args, say):
    out_dir = args.out_dir
    os.makedirs(out_dir, exist_ok=True)
    env = dict(os.environ, TMPDIR=os.environ.get('TMPDIR', '/tmp'))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', os.path.join(out_dir, 'trace'), '-o', 'bench', '--',
           sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP)]
    say('trace: rocprofv3 --kernel-trace --stats -- python bench.py ' + ' '.join(cmd[11:]))
    with open(os.path.join(out_dir, 'bench_under_rocprof.out'), 'w') as o, open(os.path.join(out_dir, 'bench_under_rocprof.err'), 'w') as e:
        rc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=o, stderr=e, timeout=args.limit).returncode
    if rc != 0:
        say('trace: rocprofv3 ended with status %d' % rc)
        return rc
    for line in open(os.path.join(out_dir, 'bench_under_rocprof.out')):
        if line.startswith('{'):
            say('trace: bench line under the profiler: ms_per_step %s' % json.loads(line).get('ms_per_step'))
    db = find_db(os.path.join(out_dir, 'trace'))
    if db is None:
        say('trace: no *_results.db under %s' % out_dir)
        return 1
    ok = analyse(db, STEPS, say)
    stats = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_stats.py'), db, '--steady', 'prefilter_scan:%d' % STEPS, '--csv',
                            os.path.join(out_dir, args.name + '_kernel_stats.csv'), '--top', '30'], capture_output=True, text=True)
    with open(os.path.join(out_dir, args.name + '_kernel_stats.txt'), 'w') as f:
        f.write(stats.stdout + stats.stderr)
    os.remove(db)                                                       # (large: the summaries are what is kept)
    return 0 if ok and stats.returncode == 0 else 1


def leg_time(args, say):
    import torch
    from odtk import _C
    dev = torch.device('cuda')
    taken = _C.library_plans_import('\n'.join(json.load(open(PLAN))['libraries']) + '\n')
    say('time: plan lines taken (gemm, conv) = %s' % (list(taken),))
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(256, 256, 3, 3, generator=g) * 0.02).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = (torch.randn(256, generator=g) * 0.1).to(dev, torch.bfloat16)

    def act(h, wd):
        return torch.randn(8, 256, h, wd, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def group(shapes):
        xs = [act(*s) for s in shapes]
        ys = [torch.empty_like(x) for x in xs]

        def run():
            for x, y in zip(xs, ys):
                _C.conv_bias_act(x, w, b, 1, 1, True, out=y)
        run()
        names = [_C.conv_last_plan()]
        return run, names

    def timed(run, reps=30):
        for _ in range(5):
            run()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        times.sort()
        return times[len(times) // 2], times[0], times[-1], times[len(times) // 4], times[3 * len(times) // 4]

    results = {}
    cases = [('P4 50x80', [LEVELS[0]]), ('P5 25x40', [LEVELS[1]]), ('P6 13x20', [LEVELS[2]]), ('P7 7x10', [LEVELS[3]]),
             ('P4..P7, four launches', LEVELS), ('canvas 50x121, one launch', [(50, 121)]),
             ('P5..P7, three launches', LEVELS[1:]), ('canvas 25x72, one launch', [(25, 72)]),
             ('P4 + canvas 25x72, two launches', [LEVELS[0], (25, 72)])]
    for name, shapes in cases:
        run, plans = group(shapes)
        results[name] = timed(run)
        say('time: %-34s median %7.1f us  (min %7.1f  max %7.1f  quartiles %7.1f .. %7.1f)   last instance: %s'
            % ((name,) + results[name] + (plans[0],)))
    for canvas, replaced in (('canvas 50x121, one launch', 'P4..P7, four launches'), ('canvas 25x72, one launch', 'P5..P7, three launches'),
                             ('P4 + canvas 25x72, two launches', 'P4..P7, four launches')):
        c, r = results[canvas], results[replaced]
        spread = max(c[4] - c[3], r[4] - r[3])
        say('time: %s saves %.1f us of %.1f per tower layer (quartile spread of the medians: %.1f us) -> %s'
            % (canvas, r[0] - c[0], r[0], spread, 'beats it' if r[0] - c[0] > spread else 'does NOT beat it'))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['all', 'trace', 'time'], default='all')
    ap.add_argument('--out', default=None, help='text report (appended by the legs)')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'build', 'pyramid_canvas_probe'))
    ap.add_argument('--name', default='parent', help='prefix of the kernel-stats files of the trace leg')
    ap.add_argument('--limit', type=int, default=420, help='seconds each leg may take')
    args = ap.parse_args()
    out = args.out or os.path.join(args.out_dir, 'pyramid_canvas_probe.txt')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def say(text):
        print(text, flush=True)
        with open(out, 'a') as f:
            f.write(text + '\n')

    if args.leg == 'all':
        for leg in ('trace', 'time'):                                   # each leg: a process of its own, its own limit, no retry
            rc = subprocess.run(['timeout', '-k', '10', str(args.limit + 60), sys.executable, os.path.abspath(__file__), '--leg', leg, '--out', out,
                                 '--out-dir', args.out_dir, '--name', args.name, '--limit', str(args.limit)]).returncode
            if rc != 0:
                say('probe: leg %s ended with status %d: stopping' % (leg, rc))
                return rc
        return 0
    return (leg_trace if args.leg == 'trace' else leg_time)(args, say)


if __name__ == '__main__':
    sys.exit(main())
