#!/usr/bin/env python3
"""The Python side of self-play against the parent commit's: bench.py as a child process, alternating parent / new, for the default
workload (device moves: SelfPlayReader.read_rows) and for the host-driven move step with and without the pipeline (the loop that keeps
its games in the book since this change).

    python profiles/ab_host_book.py --parent DIR [--out profiles/host_book/ab.txt] [--runs 3] [--configs 0,1,2] [--append]

DIR is a checkout of the parent commit; its bench.py runs there against THIS tree's library (RZ_HIP_LIBRARY: the C++ side is the
same).  Every run writes --dump-outputs, and every new run's arrays are compared bit for bit with the parent's.  The span of the
parent's own runs is the noise of the day: a new run's moves / s may be below the parent's slowest by no more than that span; every
line is written whether it holds or not.  The first child that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (('device moves (the default workload)', []),
           ('host moves, pipelined (--device-moves 0 --pipeline 1)', ['--device-moves', '0', '--pipeline', '1']),
           ('host moves, lanes finished in turn (--device-moves 0 --pipeline 0)', ['--device-moves', '0', '--pipeline', '0']))


def bench(tree, extra, limit, dump):
    env = dict(os.environ)
    env.pop('RZ_HIP_LIBRARY', None)
    if tree != REPO:
        env['RZ_HIP_LIBRARY'] = os.path.join(REPO, 'rlzero_amd', 'librlzero_hip.so')
    cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5', '--dump-outputs', dump] + extra
    done = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    if done.returncode != 0:
        sys.stderr.write(done.stderr.decode(errors='replace')[-4000:])
        raise SystemExit('bench.py ended with %d: %s' % (done.returncode, ' '.join(cmd)))
    return json.loads([ln for ln in done.stdout.decode().splitlines() if ln.startswith('{')][-1])


def arrays(path):
    return dict((n, np.load(os.path.join(path, n)).tobytes()) for n in sorted(os.listdir(path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a checkout of the parent commit')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'host_book', 'ab.txt'))
    ap.add_argument('--runs', type=int, default=3, help='runs per build and configuration')
    ap.add_argument('--limit', type=float, default=240.0, help='seconds a child may take')
    ap.add_argument('--configs', default='0,1,2')
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()
    trees = {'parent': os.path.abspath(args.parent), 'new': REPO}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    if not args.append:
        say('# profiles/ab_host_book.py: python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR [...], alternating parent / new')
    verdicts = []
    for k in [int(i) for i in args.configs.split(',')]:
        name, extra = CONFIGS[k]
        say(name)
        rate, dumps = {'parent': [], 'new': []}, {'parent': [], 'new': []}
        for i in range(args.runs):
            for build in ('parent', 'new'):
                with tempfile.TemporaryDirectory() as tmp:
                    rec = bench(trees[build], extra, args.limit, tmp)
                    dumps[build].append(arrays(tmp))
                rate[build].append(rec['moves_per_sec'])
                say('  run %d %-6s %10.2f moves/s   %8.3f ms per step   %12.1f sims/s' % (i + 1, build, rec['moves_per_sec'], rec['ms_per_step'], rec['value']))
        same = bool(dumps['parent'][0]) and all(d == dumps['parent'][0] for d in dumps['parent'] + dumps['new'])
        say('  --dump-outputs (%s) of all %d runs: %s' % (', '.join(dumps['parent'][0]), len(dumps['parent']) + len(dumps['new']),
                                                        'identical' if same else 'DIFFERENT'))
        verdicts.append(same)
        lo, hi = min(rate['parent']), max(rate['parent'])
        if len(rate['parent']) > 1:
            slower = [v for v in rate['new'] if v < lo - (hi - lo)]
            say('  parent %.2f .. %.2f moves/s (spread %.2f = %.2f %%); new %.2f .. %.2f, at least %.2f asked: %s' % (
                lo, hi, hi - lo, 100.0 * (hi - lo) / hi, min(rate['new']), max(rate['new']), lo - (hi - lo),
                'holds' if not slower else 'SLOWER: %s' % slower))
            verdicts.append(not slower)
    out.close()
    sys.exit(0 if all(verdicts) else 1)


if __name__ == '__main__':
    main()
