"""tests/mz_unfold.py without a GPU: trees built by the CPython restatement of the pseudocode (oracle.muzero_ref.run_mcts) from
random float32 network outputs, laid out in slots as the device lays them out -- ``unfold`` must hand back exactly what was
fed, and must refuse every tree that has been tampered with."""
import numpy as np
import pytest

from mz_unfold import TreeRefused, unfold
from oracle import muzero_ref as ref

NODE = np.dtype([('N', '<i4'), ('first_child', '<i4'), ('value_sum', '<f8'), ('prior', '<f8'), ('reward', '<f4'), ('pad', '<i4')])
DISCOUNT = 0.997


def build_tree(n_actions, n_sims, scale, noise, seed):
    """-> (nodes [cap], top, fed): a search of ``n_sims`` simulations fed random float32 outputs (rewards and values of
    magnitude ``scale``, both signs), in the device's layout: root = slot 0, the block of children of the i-th expansion
    (the root's is the 0-th) at 1 + A * i, a child at its parent's block + action."""
    rng = np.random.RandomState(seed)
    A = n_actions
    cfg = ref.MuZeroConfig(num_simulations=n_sims, discount=DISCOUNT)
    root = ref.Node(0)
    p0 = rng.dirichlet(np.ones(A)).astype(np.float32)
    ref.expand_node(root, None, 0.0, [float(p) for p in p0])
    if noise:
        ref.add_exploration_noise(cfg, root, [float(x) for x in rng.dirichlet(0.25 * np.ones(A))])
    fed = []

    def model(hidden, action, path):
        reward = np.float32(scale * rng.uniform(-1.0, 1.0))
        value = np.float32(scale * rng.uniform(-1.0, 1.0))
        probs = rng.dirichlet(np.ones(A)).astype(np.float32)
        fed.append((path, reward, probs, value))
        return None, float(reward), [float(p) for p in probs], float(value)

    ref.run_mcts(cfg, root, model)
    cap = 1 + A * (n_sims + 1)
    nodes = np.zeros(cap, dtype=NODE)
    nodes['N'] = -1            # (the device's arena starts as 0xff bytes)
    nodes['first_child'] = -1
    block = {(): 1}
    for i, (path, _, _, _) in enumerate(fed):
        block[path] = 1 + A * (i + 1)
    slot = {(): 0}
    for path, (n, value_sum, reward, prior) in sorted(ref.tree_dump(root).items(), key=lambda kv: len(kv[0])):
        if path:
            slot[path] = block[path[:-1]] + path[-1]
        nodes[slot[path]] = (n, block.get(path, -1), value_sum, prior, reward, 0)
    return nodes, 1 + A * (n_sims + 1), fed, [c.prior for c in root.children]


CASES = [(A, n, scale, noise) for A in (2, 3, 8) for n in (1, 2, 50) for scale in (1.0, 30.0) for noise in (False, True)]


@pytest.mark.parametrize('n_actions,n_sims,scale,noise', CASES)
def test_unfold_returns_exactly_what_the_search_was_fed(n_actions, n_sims, scale, noise):
    for seed in range(4):
        nodes, top, fed, root_prior = build_tree(n_actions, n_sims, scale, noise, 1000 * n_actions + 10 * n_sims + seed)
        got, got_root = unfold(nodes, top, n_actions, DISCOUNT)
        assert len(got) == len(fed) == n_sims
        assert [float(p).hex() for p in got_root] == [float(p).hex() for p in root_prior]
        for e, (path, reward, probs, value) in zip(got, fed):
            assert e.path == path and e.action == path[-1]
            assert e.reward.dtype == np.float32 and e.value.dtype == np.float32 and e.probs.dtype == np.float32
            assert e.reward.tobytes() == reward.tobytes() and e.value.tobytes() == value.tobytes()
            assert e.probs.tobytes() == probs.tobytes()
            parent = 0
            for a in path[:-1]:
                parent = int(nodes['first_child'][parent]) + a
            assert e.parent == parent and e.slot == int(nodes['first_child'][parent]) + path[-1]


def _expanded(nodes, top):
    return [s for s in range(top) if nodes['first_child'][s] >= 0]


@pytest.mark.parametrize('n_actions,scale', [(2, 1.0), (2, 30.0), (3, 1.0), (8, 30.0)])
def test_unfold_refuses_a_tree_that_was_tampered_with(n_actions, scale):
    nodes, top, fed, _ = build_tree(n_actions, 50, scale, True, 77 + n_actions)
    unfold(nodes, top, n_actions, DISCOUNT)   # the honest tree decodes
    rng = np.random.RandomState(5)
    expanded = _expanded(nodes, top)
    visited = [s for s in range(top) if nodes['N'][s] > 0]

    values = {e.slot: e.value for e in unfold(nodes, top, n_actions, DISCOUNT)[0]}

    def off_grid(shift, v32):   # `shift` moves a value away from the float32 grid: between 1/4 and 3/4 of an ulp past a whole number
        return 0.25 <= (abs(shift) / float(np.spacing(np.abs(np.float32(v32))))) % 1.0 <= 0.75

    # one value_sum moved by 1e-6.  The root's enters the root identity (1e-9 relative).  Any other node's moves that node's own
    # recovered value by 1e-6: refused for certain where 1e-6 is not (nearly) a whole number of that value's float32 ulps --
    # where it is, the moved sum spells another float32 and only the parent's identity is left to object.
    # (At output scale 30 the root's sum is in the thousands and 1e-6 of it is inside that 1e-9: the root is moved at scale 1.)
    root = [0] if abs(nodes['value_sum'][0]) < 500.0 else []
    assert root or scale > 1.0
    targets = [s for s in visited[1:] if off_grid(1e-6, values[s])]
    assert len(targets) >= 12
    for s in root + [int(x) for x in rng.choice(targets, size=12, replace=False)]:
        for delta in (1e-6, -1e-6):
            bad = nodes.copy()
            bad['value_sum'][s] += delta
            with pytest.raises(TreeRefused):
                unfold(bad, top, n_actions, DISCOUNT)

    # one N off by one
    for s in [0] + [int(x) for x in rng.choice(np.arange(1, top), size=12, replace=False)]:
        for delta in (1, -1):
            bad = nodes.copy()
            bad['N'][s] += delta
            with pytest.raises(TreeRefused):
                unfold(bad, top, n_actions, DISCOUNT)

    # two first_child values swapped: two expanded nodes, and an expanded node with one that is not
    # (two nodes with the SAME visit count can trade their blocks and leave every count right -- two nodes visited once
    # describe, traded, the same search with two simulations in the other order; the replay of the pseudocode is what objects
    # to that one, tests/test_muzero_moves_tree.py -- so the pairs here differ in N)
    done = 0
    while done < 12:
        a, b = (int(x) for x in rng.choice(expanded, size=2, replace=False))
        if nodes['N'][a] == nodes['N'][b]:
            continue
        done += 1
        bad = nodes.copy()
        bad['first_child'][a], bad['first_child'][b] = nodes['first_child'][b], nodes['first_child'][a]
        with pytest.raises(TreeRefused):
            unfold(bad, top, n_actions, DISCOUNT)
    leaves = [s for s in range(top) if nodes['first_child'][s] < 0]
    for _ in range(6):
        a, b = int(rng.choice(expanded)), int(rng.choice(leaves))
        bad = nodes.copy()
        bad['first_child'][a], bad['first_child'][b] = nodes['first_child'][b], nodes['first_child'][a]
        with pytest.raises(TreeRefused):
            unfold(bad, top, n_actions, DISCOUNT)

    # one reward changed.  A reward enters ONE identity, its parent's.  Below the root the check on that identity is that the
    # parent's recovered value is a float32, so a change is caught unless N_c * (change) happens to move the parent's value
    # onto another float32 -- then the tree IS a tree the kernel could have written, from another network output.  The changes
    # made here are the smallest there are (the next float32) on nodes where that cannot happen: visited once, with a reward
    # whose ulp is 1/2 or 1/4 of the ulp of the parent's value (the value moves by that fraction of its ulp).
    fc = nodes['first_child']
    root_kids = [int(fc[0]) + a for a in range(n_actions) if nodes['N'][int(fc[0]) + a] > 0]
    for c in root_kids:   # a child of the root: the root identity holds to 1e-9
        bad = nodes.copy()
        bad['reward'][c] = np.float32(nodes['reward'][c]) * np.float32(1.001) + np.float32(1e-3)
        with pytest.raises(TreeRefused):
            unfold(bad, top, n_actions, DISCOUNT)
    deep = []
    for p in expanded[1:]:
        for a in range(n_actions):
            c = int(fc[p]) + a
            ratio = float(np.spacing(np.abs(values[p]))) / float(np.spacing(np.abs(np.float32(nodes['reward'][c]))))
            if nodes['N'][c] == 1 and ratio in (2.0, 4.0):
                deep.append(c)
    assert len(deep) >= 3
    for c in deep[:8]:
        for toward in (np.float32(np.inf), np.float32(-np.inf)):
            bad = nodes.copy()
            bad['reward'][c] = np.nextafter(np.float32(nodes['reward'][c]), toward)
            if np.spacing(np.abs(bad['reward'][c])) != np.spacing(np.abs(nodes['reward'][c])):
                continue   # (stepped across a power of two: another ulp)
            with pytest.raises(TreeRefused):
                unfold(bad, top, n_actions, DISCOUNT)
    # ... and a reward on a node that was never visited
    bad = nodes.copy()
    bad['reward'][leaves[-1]] = 0.5
    with pytest.raises(TreeRefused):
        unfold(bad, top, n_actions, DISCOUNT)
