"""Writes agreement.txt: per route of tests/test_noise_streams_gpu.py the tolerance the test computed on the CPU (T_rel = 4 x the
restatement's own float32-vs-float64 spread on the test's keys) and what the device showed.  Needs an MI355X; run once from the
repository root:

    python profiles/noise_streams/measure.py [--out profiles/noise_streams/agreement.txt]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'agreement.txt'))
    args = ap.parse_args()
    import pytest
    os.chdir(REPO)
    rc = pytest.main(['-q', '-m', 'gpu', '-p', 'no:cacheprovider', os.path.join('tests', 'test_noise_streams_gpu.py')])
    measured = sys.modules['test_noise_streams_gpu'].MEASURED
    lines = ['Device noise streams against tests/device_streams.py on an MI355X (pytest exit code %d).' % int(rc),
             'AlphaZero / MuZero noise: T_rel = tolerance computed on the CPU; observed = worst relative difference of the device',
             '(AlphaZero: beyond the read-back resolution R = 4 ulp(prior) / 0.25); samples = nodes or moves; left out = share with an',
             'acceptance margin below 1e-4.  Action draws: observed = share of the records that differ from the restatement.', '',
             '%-66s %11s %11s %9s %9s' % ('route', 'T_rel', 'observed', 'samples', 'left out')]
    for route in sorted(measured):
        t_rel, seen, n, share = measured[route]
        lines.append('%-66s %11.3e %11.3e %9d %8.2f%%' % (route, t_rel, seen, n, 100.0 * share))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return int(rc)


if __name__ == '__main__':
    sys.exit(main())
