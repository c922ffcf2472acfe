"""
Signed rows: forward kernels whose row tiles can be two-coloured generate the rows of one colour with the sign of
psky in their weight and drop the XOR mask on the off-diagonal tiles.  Every shape that takes the rule (the pair kernel with and without
hub and FLAT, the pair cross kernel, the generic cross shapes 32 x 32, 32 x 64, 64 x 64 and 128 x 128) -- and the generic two-tile diagonal
shapes next to them -- on the MI355X against the float64 vector-ALU kernels, at the max-norm tolerance of the pair-form tests
(1e-5), two runs bit for bit.  psky has mixed signs within a row, one all-negative row and one all-positive row in the same call,
so that the signed and the unsigned instantiation run side by side.  704 directions (22 panels), Nf = 3, Nt = 2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bayeslim_amd import utils
from pair_cross_cases import make_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
NT, NF, P = 2, 3, 704
TOL = 1e-5


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def hex127_hub(z_offsets=False):
    """hex-127 + an outrigger; with z_offsets the mirror pairs leave the plane by an odd function of the position (point symmetry
    kept, no `flat` licence)"""
    ant = np.vstack([utils._make_hex(7, D=14.6)[1], [[250.0, 0.0, 0.0]]])
    if z_offsets:
        ant[:, 2] = 0.5 * np.sin(0.013 * ant[:, 0] + 0.007 * ant[:, 1])
    return ant


def symmetric(firsts, singles, seed):
    rng = np.random.default_rng(seed)
    h = rng.normal(0, 70.0, (firsts, 3)) * [1, 1, 0.05]
    ant = np.vstack([h, -h] + ([rng.normal(0, 70.0, (singles, 3)) * [1, 1, 0.05]] if singles else []))
    return ant[rng.permutation(len(ant))] + [31.7, -12.3, 4.1]


def plain(n, seed):
    return np.random.default_rng(seed).normal(0, 70.0, (n, 3)) * [1, 1, 0.05]


def inputs(ant, seed):
    """the full pair set in antenna order, unit directions of the upper half sky, psky (Nt, 1, 1, Nf, P) float64"""
    rng = np.random.default_rng(seed)
    n = len(ant)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    blvecs = T64(np.stack([ant[b] - ant[a] for a, b in pairs])).cuda()
    freqs = T64(np.linspace(120e6, 180e6, NF))
    s = rng.normal(size=(NT, 3, P))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[:, 2] = np.abs(s[:, 2])
    shape = (NT, 1, 1, NF, P)
    psky = rng.normal(size=shape) * np.exp(-9.0 * rng.uniform(size=shape))
    psky[0, :, :, 1] = -np.abs(psky[0, :, :, 1])         # every sign set
    psky[1, :, :, 2] = np.abs(psky[1, :, :, 2])          # no sign: the mask-free instantiation
    return pairs, blvecs, freqs, T64(s).cuda(), T64(psky).cuda()


def both(ops, ant, seed, check_plan=None, **geom_kw):
    """(matrix-core visibilities, float64 vector-ALU visibilities, geometry); two matrix-core runs bit-identical"""
    pairs, blvecs, freqs, sdir, psky = inputs(ant, seed)
    geom = ops.FringeGeometry(blvecs, sdir, freqs, antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True, **geom_kw)
    assert geom.ant is not None
    if check_plan is not None:
        check_plan(geom)
    ref = ops.fringe_sum(psky, ops.FringeGeometry(blvecs, sdir, freqs, mfma=False))
    assert ref.dtype == torch.complex128
    x = psky.float()
    out = [ops.fringe_sum(x, geom).clone() for _ in range(2)]
    assert torch.equal(out[0], out[1])
    return out[0], ref, geom


def relmax(a, b):
    return float((a.to(torch.complex128) - b).abs().max() / b.abs().max())


def blocks_of(geom):
    return geom.ant.get('blocks_real', geom.ant['blocks'])


_REF = {}


def hub_case(ops):
    """hex-127 + outrigger + hub, computed once for the two tests that look at it"""
    if 'hub' not in _REF:
        def plan(geom):
            assert geom.ant['pair_blocks'] == [(63, 64, 1)], geom.ant['pair_blocks']
            assert blocks_of(geom)[0]['flat']
        _REF['hub'] = both(ops, hex127_hub(), 101, plan)
    return _REF['hub']


def test_pair_kernel_with_hub_flat(ops):
    """pair kernel, CEN, FLAT: 63 pairs + the outrigger in 64 rows, the hub in the column sums"""
    vis, ref, _ = hub_case(ops)
    err = relmax(vis, ref)
    print('hex127 + outrigger + hub: max |vis - float64| / max |vis| = %.2e' % err)
    assert err < TOL


def test_hub_column_sums_on_their_own(ops):
    """the `centre` baselines alone: column sums over rows of both colours with mixed-sign weights"""
    vis, ref, geom = hub_case(ops)
    cen = blocks_of(geom)[0]['centre']
    slots = torch.unique(cen[cen >= 0]).to(torch.int64)
    assert len(slots) == 127                             # the hub against the 126 paired antennas and the outrigger
    err = relmax(vis[:, slots], ref[:, slots])
    print('hub baselines: max |vis - float64| / max |vis| = %.2e' % err)
    assert err < TOL


def test_pair_kernel_with_hub_not_flat(ops):
    """the same array with z offsets on the mirror pairs: FLAT false"""
    def plan(geom):
        assert geom.ant['pair_blocks'] == [(63, 64, 1)], geom.ant['pair_blocks']
        assert not blocks_of(geom)[0]['flat']
    vis, ref, _ = both(ops, hex127_hub(z_offsets=True), 102, plan)
    err = relmax(vis, ref)
    print('hex127 + outrigger + hub, z offsets: %.2e' % err)
    assert err < TOL


@pytest.mark.parametrize('firsts', [40, 33])
def test_pair_kernel_without_hub(ops, firsts):
    """a random point-symmetric array: 40 firsts (tile 1 partly padded) and 33 (one row in tile 1), no hub"""
    def plan(geom):
        assert geom.ant['pair_blocks'] == [(firsts, firsts, 0)], geom.ant['pair_blocks']
    vis, ref, _ = both(ops, symmetric(firsts, 0, 103 + firsts), 104, plan)
    err = relmax(vis, ref)
    print('%d mirror pairs: %.2e' % (firsts, err))
    assert err < TOL


@pytest.mark.parametrize('kind', ['hex169', 'rand200'])
def test_pair_cross_blocks(ops, kind):
    """hex-169, and 200 random antennas with rows that have no partner: the pair cross kernel between the symmetric groups"""
    def plan(geom):
        assert geom.ant.get('pair_cross_blocks'), geom.ant.get('pair_cross_blocks')
        assert any(b.get('xpair') for b in blocks_of(geom))
    vis, ref, _ = both(ops, make_array(kind, np.random.default_rng(105)), 106, plan)
    err = relmax(vis, ref)
    print('%s: %.2e' % (kind, err))
    assert err < TOL


def test_generic_two_tile_diagonal(ops):
    """64 random antennas without symmetry: the generic two-tile diagonal block"""
    def plan(geom):
        blocks = blocks_of(geom)
        assert not geom.ant.get('pair_blocks') and len(blocks) == 1
        assert blocks[0]['nrows'] == 64 and blocks[0]['cross'] == 0 and not blocks[0].get('pair') and blocks[0]['mf_fwd'] == 26
    vis, ref, _ = both(ops, plain(64, 107), 108, plan)
    err = relmax(vis, ref)
    print('64 plain antennas: %.2e' % err)
    assert err < TOL


@pytest.mark.parametrize('n,group,shapes', [(64, 32, [(32, 32)]), (160, 64, [(32, 64), (64, 64)]), (150, None, [(128, 128)]),
                                            (260, None, [(128, 128)])])
def test_generic_cross_blocks(ops, n, group, shapes):
    """random antennas without symmetry, cut into groups of 32 (64 antennas: cross shape 32 x 32, K split over the waves), of
    64 (160 antennas, groups 64 + 64 + 32: 32 x 64 and 64 x 64, the four-wave mapping) and of 128 (150 and 260 antennas: 128 x 128,
    the eight-wave mapping): every generic cross shape, each asserted in the plan"""
    seen = []

    def plan(geom):
        blocks = blocks_of(geom)
        assert not geom.ant.get('pair_blocks') and not any(b.get('xpair') or b.get('pair') for b in blocks)
        seen.extend(sorted({(b['cross'], b['nrows'] - b['cross']) for b in blocks if b['cross']}))
        assert seen == shapes, (seen, shapes)
    vis, ref, _ = both(ops, plain(n, 109 + n), 110, plan, **({} if group is None else dict(group=group)))
    err = relmax(vis, ref)
    print('%d plain antennas, group %s, cross shapes %s: %.2e' % (n, group, seen, err))
    assert err < TOL


_UNPACKED_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
from bayeslim_amd import ops
import test_signed_rows_gpu as m
assert not ops.FWD_PACKED
def plan(geom):
    blocks = m.blocks_of(geom)
    assert len(blocks) == 1 and blocks[0]['nrows'] == 50 and blocks[0]['cross'] == 0 and blocks[0]['mf_fwd'] == 26, blocks[0]['mf_fwd']
vis, ref, _ = m.both(ops, m.plain(50, 111), 112, plan)
print('ERR %%.3e' %% m.relmax(vis, ref))
'''


def test_generic_two_tile_diagonal_unpacked():
    """50 random antennas with RIME_FWD_PACKED=0 (read once, when the library loads: a fresh child process): the generic two-tile
    diagonal block with a partly padded second tile, in place of the packed 33..48 kernel's neighbour"""
    env = dict(os.environ, RIME_FWD_PACKED='0')
    r = subprocess.run([sys.executable, '-c', _UNPACKED_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    err = float([ln for ln in r.stdout.splitlines() if ln.startswith('ERR')][0].split()[1])
    print('50 plain antennas, unpacked: %.2e' % err)
    assert err < TOL
