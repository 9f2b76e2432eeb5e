#!/usr/bin/env python3
"""The host side of the library against the parent commit's: bench.py as a child process, three runs per build, alternating, for the
headline workload and for one step-by-step route (several ABI calls per simulation: the host path decides more of it).

    python profiles/ab_host_runtime.py --parent-lib DIR/librlzero_hip.so [--out profiles/host_runtime/ab.txt] [--runs 3] [--configs 0,1] [--append]

The parent's library is a build of the parent commit (the same ABI); a child gets it through RZ_HIP_LIBRARY, as in the other
profiles/ab_*.py.  For every configuration: the span of the parent's own runs is the noise of the day; the new build's runs are held
against that span widened by itself on each side, and every line is written whether it falls inside or not.  One more run per build
writes --dump-outputs, and the arrays are compared bit for bit.  The first child that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (('headline (resident search, device moves)', []),
           ('step by step (--deferred 0 --graph 0: trunk, FC GEMM and tree step launched one by one)', ['--deferred', '0', '--graph', '0']))


def bench(extra, parent_lib, limit, dump=None):
    env = dict(os.environ)
    env.pop('RZ_HIP_LIBRARY', None)
    if parent_lib:
        env['RZ_HIP_LIBRARY'] = parent_lib
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'] + extra
    if dump:
        cmd += ['--dump-outputs', dump]
    done = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    if done.returncode != 0:
        sys.stderr.write(done.stderr.decode(errors='replace')[-4000:])
        raise SystemExit('bench.py ended with %d: %s' % (done.returncode, ' '.join(cmd)))
    lines = [ln for ln in done.stdout.decode().splitlines() if ln.startswith('{')]
    return json.loads(lines[-1])


def same_arrays(a, b):
    import numpy as np
    names = sorted(os.listdir(a))
    if names != sorted(os.listdir(b)) or not names:
        return False, names
    return all(np.load(os.path.join(a, n)).tobytes() == np.load(os.path.join(b, n)).tobytes() for n in names), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, help='librlzero_hip.so built from the parent commit')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'host_runtime', 'ab.txt'))
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--limit', type=float, default=240.0, help='seconds a child may take')
    ap.add_argument('--configs', default='0,1', help='which of the two configurations; with --append a second call adds to the file of the first')
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_host_runtime.py: python bench.py --gpus 1 --steps 20 --warmup 5 [...], %d runs per build, alternating parent / new' % args.runs)
    verdicts = []
    for name, extra in [CONFIGS[int(i)] for i in args.configs.split(',')]:
        say('%s' % name)
        got = {'parent': [], 'new': []}
        for i in range(args.runs):
            for build in ('parent', 'new'):
                rec = bench(extra, parent if build == 'parent' else None, args.limit)
                got[build].append(rec['value'])
                say('  run %d %-6s %12.1f sims/s   %8.3f ms per step   engine_hbm_bytes %s' % (
                    i + 1, build, rec['value'], rec['ms_per_step'], rec.get('engine_hbm_bytes', rec.get('config', {}).get('engine_hbm_bytes'))))
        lo, hi = min(got['parent']), max(got['parent'])
        span = hi - lo
        outside = [v for v in got['new'] if not lo - span <= v <= hi + span]
        say('  parent %.1f .. %.1f sims/s (span %.1f = %.2f %%); allowed %.1f .. %.1f; new %.1f .. %.1f: %s' % (
            lo, hi, span, 100.0 * span / hi, lo - span, hi + span, min(got['new']), max(got['new']),
            'all inside' if not outside else 'OUTSIDE: %s' % outside))
        verdicts.append(not outside)
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            bench(extra, parent, args.limit, dump=a)
            bench(extra, None, args.limit, dump=b)
            same, names = same_arrays(a, b)
            say('  --dump-outputs (%s): %s' % (', '.join(names), 'identical' if same else 'DIFFERENT'))
            verdicts.append(same)
    out.close()
    sys.exit(0 if all(verdicts) else 1)


if __name__ == '__main__':
    main()
