"""
Arrays and baseline sets of the pair cross block tests (tests/test_pair_cross_plan.py on the host, tests/test_pair_cross_gpu.py
on the GPU): point-symmetric arrays of more than 128 antennas, and the ground that must not move.  numpy only.
"""
import zlib

import numpy as np

CENTRE = np.array([31.7, -12.3, 4.1])

# kind -> expected plan: ([(pairs, rows, hub) of the groups' diagonal blocks], [(rows_i, rows_j) of the cross blocks]); None: declines
EXPECTED = {
    'hex169': ([(43, 43, 0), (41, 42, 0)], [(43, 42)]),
    'hex217': ([(55, 55, 0), (53, 54, 0)], [(55, 54)]),
    'hex271': ([(46, 46, 0), (46, 46, 0), (43, 44, 0)], [(46, 46), (46, 44), (46, 44)]),
    'hex169t': ([(43, 43, 0), (41, 42, 0)], [(43, 42)]),
    'rand200': ([(55, 55, 0), (35, 55, 0)], [(55, 55)]),
    'hex127+1': None,
    'rand128': None,
    'plain150': None,
}
CROSS_KINDS = [k for k, v in EXPECTED.items() if v is not None]
UNCHANGED_KINDS = [k for k, v in EXPECTED.items() if v is None]


def seed_of(kind, extra=0):
    return zlib.crc32(kind.encode()) % 1000 + extra


def make_array(kind, rng):
    """antenna positions (n, 3): hexagons as the generator makes them (hex169 / 217 / 271: 8 / 9 / 10 on a side), `t`: tilted out
    of the plane z = const (no `flat` licence); rand200: 90 mirror pairs + 20 antennas without a partner with a z spread;
    rand128: 60 pairs + 8 singles; plain150: no symmetry.  Rows permuted, centre away from the origin."""
    from bayeslim_amd import utils
    if kind.startswith('hex'):
        side, extra = {'hex169': (8, 0), 'hex217': (9, 0), 'hex271': (10, 0), 'hex127+1': (7, 1)}[kind.rstrip('t')]
        ant = utils._make_hex(side, D=14.6)[1]
        if extra:
            ant = np.vstack([ant, [[250.0, 3.0, 0.0]]])
        if kind.endswith('t'):
            t = np.deg2rad(3.0)
            ant = ant @ np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]]).T
    elif kind == 'plain150':
        ant = rng.normal(0, 90.0, (150, 3)) * [1, 1, 0.05]
    else:
        half, single = {'rand200': (90, 20), 'rand128': (60, 8)}[kind]
        h = rng.normal(0, 90.0, (half, 3)) * [1, 1, 0.05]
        ant = np.vstack([h, -h, rng.normal(0, 90.0, (single, 3)) * [1, 1, 0.05]])
    return ant[rng.permutation(len(ant))] + CENTRE


def make_pairs(n, rng, full):
    """the full pair set in antenna order, or a 90 % subset with mixed orientations plus a few autocorrelations, shuffled"""
    if full:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs = [(i, j) if rng.random() < 0.5 else (j, i) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.9]
    pairs += [(a, a) for a in range(n) if a % 40 == 3]
    return [pairs[k] for k in rng.permutation(len(pairs))]
