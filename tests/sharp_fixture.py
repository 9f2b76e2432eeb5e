"""Loaders of the g9 fixtures (tests/golden/gen_golden.py g9): boards of 11, 15 and 16 rows on oracle.evaluators.sharp_weights, whose
values spread over (-1, 1) -- recorded runs of the reference's own net and search.  Shared by tests/test_sharp_fixture.py (CPU),
tests/test_sharp_net_rows.py (GPU) and profiles/sharp_net_agreement.py; every tolerance comes from here, none from a device."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BOARDS = (11, 15, 16)
E_VALUE_MAX, E_LOGP_MAX = 2e-6, 2e-5   # the suite's tight bounds (the heads test): E and E_lp may never exceed them

_cache = {}


def _json(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, name + '.json.gz'), 'rb') as f:
            _cache[name] = json.loads(f.read().decode())
    return _cache[name]


def search(B):
    """{'seed', 'gain', 'e_value', 'e_logp' (hex), 'margin', 'stats', 'cases': [...]} of one board."""
    key = ('search', B)
    if key not in _cache:
        parts = [_json('g9_sharpsearch_B%d_%d' % (B, k)) for k in range(2)]
        assert all({k: v for k, v in p.items() if k != 'cases'} == {k: v for k, v in parts[0].items() if k != 'cases'} for p in parts)
        _cache[key] = dict(parts[0], cases=[c for p in parts for c in p['cases']])
    return _cache[key]


def games():
    return _json('g9_sharpgames')['games']


def net(B):
    """The 24 positions of a board: planes float32 [24,4,B,B], move lists, the reference's log_probs [24,S] and value [24]."""
    key = ('net', B)
    if key not in _cache:
        z = np.load(os.path.join(GOLDEN, 'g9_sharpnet_B%d.npz' % B))
        planes = np.unpackbits(z['plane_bits'], axis=2)[:, :, :B * B].reshape(-1, 4, B, B).astype(np.float32)
        moves = [[int(m) for m in row if m >= 0] for row in z['moves']]
        _cache[key] = {'planes': planes, 'moves': moves, 'log_probs': z['log_probs'], 'value': z['value'],
                       'e_value': float(z['e_value']), 'e_logp': float(z['e_logp'])}
    return _cache[key]


def weights(B):
    from oracle.evaluators import sharp_weights
    head = search(B)
    return sharp_weights(B, head['seed'], head['gain'])


def tolerances(B):
    """(E, E_lp) = margin x the measured max |torch f32 - torch f64| over every recorded position and leaf of the board."""
    head = search(B)
    return head['margin'] * float.fromhex(head['e_value']), head['margin'] * float.fromhex(head['e_logp'])


def leaf_values(rec):
    return [float.fromhex(v) for _, v in rec['leaves']]
