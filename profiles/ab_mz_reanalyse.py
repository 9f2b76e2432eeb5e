#!/usr/bin/env python3
"""What MuZero Reanalyse costs (rlzero_amd/muzero/reanalyse.py), in one process, HIP events on the launch stream, medians after warm-up.

  refresh     8192 CartPole environments fill a MuZeroDeviceReplay of 2000 episodes (whole moves, the hand-over on the device); a
              MuZeroReanalyser(n_sims 50, batch 2048) then refreshes 256, 2048 and 16384 positions drawn on the device, the three
              sizes alternating, --reps times each.  Events between the stages of every chunk give the split: positions (one
              launch per refresh) | initial inference | search | read-out + update, summed over the refresh's chunks.
  iteration   the learner iteration of tools/train_muzero.py (MuZeroPipeline: collect 20 moves, [refresh], 40 updates of batch 256)
              at 8192 environments, one event pair around each iteration: off | --reanalyse 2048 | --reanalyse all | the parent
              commit (--parent DIR: a checkout of it with its library built, loaded beside this tree's package under another
              name; run TWICE, as two pipelines, so that the spread between two runs of the same code stands next to the
              difference off - parent).  All pipelines start from the same seed and alternate iteration by iteration.
  learning    ONE observation, no claim: MuZeroPipeline(256 environments, device replay).run(60) with and without reanalyse='all',
              same seed; the final episode_len of each (and of reanalyse=2048).

    python profiles/ab_mz_reanalyse.py [--out profiles/mz_reanalyse/ab.txt] [--reps 30] [--parent DIR] [--parts refresh,iteration,learning]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import contextlib
import importlib.util
import io
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ('positions', 'inference', 'search', 'update')


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


class StageEvents(object):
    """MuZeroReanalyser.timer: an event on the stream at every mark; ``take`` -> ms per stage (summed over chunks) and in all."""

    def __init__(self, torch):
        self.torch, self.marks = torch, []

    def __call__(self, label):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append((label, ev))

    def take(self):
        self.torch.cuda.synchronize()
        out = dict.fromkeys(STAGES, 0.0)
        for (_, a), (label, b) in zip(self.marks, self.marks[1:]):
            out[label] += a.elapsed_time(b)
        out['total'] = self.marks[0][1].elapsed_time(self.marks[-1][1])
        self.marks = []
        return out


def load_trainer(repo, package_name):
    """tools/train_muzero.py of the checkout ``repo`` with ``rlzero_amd`` meaning that checkout's package (loaded as
    ``package_name``, so that two checkouts live in one process: the package imports its own modules relatively and finds its
    library beside itself)."""
    if package_name != 'rlzero_amd':
        spec = importlib.util.spec_from_file_location(package_name, os.path.join(repo, 'rlzero_amd', '__init__.py'),
                                                      submodule_search_locations=[os.path.join(repo, 'rlzero_amd')])
        pkg = importlib.util.module_from_spec(spec)
        sys.modules[package_name] = pkg
        spec.loader.exec_module(pkg)
        importlib.import_module(package_name + '.muzero')
    spec = importlib.util.spec_from_file_location('train_muzero_' + package_name, os.path.join(repo, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    spec.loader.exec_module(mod)
    sys.path[:] = path   # (the script puts its own checkout first)

    @contextlib.contextmanager
    def as_rlzero_amd():   # the script's `from rlzero_amd.muzero import ...` runs when a pipeline is made
        keep = {k: v for k, v in sys.modules.items() if k == 'rlzero_amd' or k.startswith('rlzero_amd.')}
        if package_name != 'rlzero_amd':
            for k in keep:
                del sys.modules[k]
            for k, v in list(sys.modules.items()):
                if k == package_name or k.startswith(package_name + '.'):
                    sys.modules['rlzero_amd' + k[len(package_name):]] = v
        try:
            yield
        finally:
            if package_name != 'rlzero_amd':
                for k in [k for k in sys.modules if k == 'rlzero_amd' or k.startswith('rlzero_amd.')]:
                    del sys.modules[k]
                sys.modules.update(keep)
    return mod, as_rlzero_amd


def part_refresh(args, torch, say):
    from rlzero_amd.muzero import CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroReanalyser, MuZeroSelfPlay
    torch.manual_seed(args.seed)
    agent = MuZeroAgent(device='cuda:0')
    env = CartPoleBatch(args.envs, 'cuda:0', seed=args.seed)
    sp = MuZeroSelfPlay(agent.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(4, 2, 2000, int(env.max_episode_steps), device='cuda:0', seed=args.seed)
    sp.collect(48, replay=dev)
    sp.close()
    rean = MuZeroReanalyser(agent.net, dev, n_sims=args.sims, batch=args.batch, seed=args.seed)
    rean.timer = StageEvents(torch)
    sizes = (256, 2048, 16384)
    say('refresh: %d episodes held (%d steps), n_sims %d, batch %d, fused search %s; ms per refresh, %d repetitions, the sizes alternating' % (
        len(dev), int(dev.lengths().sum()), args.sims, args.batch, rean.fused, args.reps))
    for _ in range(3):
        for n in sizes:
            rean.reanalyse_sample(n)
            rean.timer.take()
    got = {n: [] for n in sizes}
    wall = {n: [] for n in sizes}
    for _ in range(args.reps):
        for n in sizes:
            t0 = time.perf_counter()
            rean.reanalyse_sample(n)
            got[n].append(rean.timer.take())
            wall[n].append(1e3 * (time.perf_counter() - t0))
    for n in sizes:
        med = {k: statistics.median(r[k] for r in got[n]) for k in STAGES + ('total', )}
        say('  %5d positions (%d chunks): events first to last %s | host clock incl. synchronise median %.3f' % (
            n, -(-n // args.batch), spread([r['total'] for r in got[n]]), statistics.median(wall[n])))
        say('        medians: positions %.3f | initial inference %.3f | init_roots + search %.3f | read-out + update %.3f   (%.1f M simulations/s over the '
            'search stage, padded rows included)' % (med['positions'], med['inference'], med['search'], med['update'],
                                                     -(-n // args.batch) * args.batch * args.sims / med['search'] / 1e3))
    rean.close()
    dev.close()


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    variants = [('off', here, as_here, {}), ('--reanalyse 2048', here, as_here, dict(reanalyse=2048)),
                ('--reanalyse all', here, as_here, dict(reanalyse='all'))]
    if args.parent:
        parent, as_parent = load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        variants += [('parent commit (1)', parent, as_parent, {}), ('parent commit (2)', parent, as_parent, {})]
    pipes = []
    for name, mod, ctx, kw in variants:
        torch.manual_seed(args.seed)
        with ctx():
            pipes.append(mod.MuZeroPipeline(n_envs=args.envs, n_sims=args.sims, batch_size=256, updates_per_iteration=40, device_replay=True,
                                            seed=args.seed, **kw))

    def iteration(pipe):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pipe.collect_selfplay_data()
        if hasattr(pipe, 'reanalyse_targets'):
            pipe.reanalyse_targets()
        pipe.policy_update()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        for pipe in pipes:
            iteration(pipe)
    ms = [[] for _ in pipes]
    for _ in range(args.reps):
        for i, pipe in enumerate(pipes):
            ms[i].append(iteration(pipe))
    say('iteration: %d environments, collect %d moves, 40 updates of batch 256; ms per iteration, %d repetitions after 3, the pipelines '
        'alternating' % (args.envs, pipes[0].moves_per_iteration, args.reps))
    med = {}
    for (name, _, _, _), pipe, xs in zip(variants, pipes, ms):
        med[name] = statistics.median(xs)
        extra = ''
        if getattr(pipe, 'reanalyser', None) is not None:
            extra = '   (%.0f positions refreshed per iteration, buffer of %d steps at the end)' % (
                pipe.reanalyser.positions_done / (args.reps + 3.0), int(pipe.buffer.lengths().sum()))
        say('  %-18s %s%s' % (name, spread(xs), extra))
    if args.parent:
        a, b = med['parent commit (1)'], med['parent commit (2)']
        say('  two runs of the parent commit differ by %.3f ms (medians %.3f and %.3f); off - parent (1) = %+.3f ms, off - parent (2) = %+.3f ms: '
            'off lies %s the parent runs\' spread' % (abs(a - b), a, b, med['off'] - a, med['off'] - b,
                                                     'inside' if min(a, b) - abs(a - b) <= med['off'] <= max(a, b) + abs(a - b) else 'OUTSIDE'))
    else:
        say('  parent commit: not measured (no --parent)')


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation per variant, same seed; no claim): MuZeroPipeline(256 environments, device replay).run(60)')
    for name, kw in (('without reanalyse', {}), ('reanalyse 2048', dict(reanalyse=2048)), ('reanalyse all', dict(reanalyse='all'))):
        torch.manual_seed(args.seed)
        with as_here():
            pipe = here.MuZeroPipeline(device_replay=True, seed=args.seed, **kw)
        t0 = time.perf_counter()
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            final = pipe.run(60)
        torch.cuda.synchronize()
        lens = [line.split('episode_len:')[1].split(',')[0] for line in log.getvalue().splitlines() if 'episode_len:' in line]
        say('  %-18s final episode_len %.1f   (%.1f s for the 60 iterations; episode_len every 10th iteration: %s)' % (
            name, final, time.perf_counter() - t0, ' '.join(lens[9::10])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_reanalyse', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='refresh,iteration,learning')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_reanalyse.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_reanalyse.py --parts %s: %s; HIP events on the launch stream unless a line says otherwise' % (
        args.parts, torch.cuda.get_device_name(0)))
    for part in args.parts.split(','):
        {'refresh': part_refresh, 'iteration': part_iteration, 'learning': part_learning}[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
