"""
The pair backward kernel with rotated phasors (round 6) on the MI355X: hex-127 + outrigger (hub path, two row
tiles) and hex-37 (one row tile) in the benchmark's antenna numbering -- the numbering whose rows form progressions -- against
the float64 vector-ALU kernels, both fringe signs, with the hub and without, full and partial baseline sets of mixed
orientation, twice bit for bit; and a random symmetric array, where RIME_PAIR_AP must not change a bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bayeslim_amd import utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def _array(kind):
    side = {'hex127': 7, 'hex127+1': 7, 'hex37': 4}[kind]
    ant = utils._make_hex(side, D=14.6)[1]
    if kind.endswith('+1'):
        ant = np.vstack([ant, [[250.0, 0.0, 0.0]]])
    return ant


def _inputs(ant, Nt, Nf, P, seed, full):
    rng = np.random.default_rng(seed)
    n = len(ant)
    if full:
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    else:
        pairs = [(i, j) if rng.random() < 0.5 else (j, i) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.9]
        pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    blvecs = T64(np.stack([ant[b] - ant[a] for a, b in pairs])).cuda()
    freqs = T64(np.linspace(120e6, 180e6, Nf))
    s = rng.normal(size=(Nt, 3, P))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[:, 2] = np.abs(s[:, 2])
    g = rng.normal(size=(1, len(pairs), Nt, Nf)) + 1j * rng.normal(size=(1, len(pairs), Nt, Nf))
    return pairs, blvecs, freqs, T64(s).cuda(), torch.as_tensor(g).cuda()


@pytest.mark.parametrize('kind,rows,hub,min_octets', [('hex127+1', 64, 1, 6), ('hex127', 64, 0, 6), ('hex37', 19, 0, 1)])
@pytest.mark.parametrize('conj', [False, True])
@pytest.mark.parametrize('full', [True, False])
def test_pair_backward_rotated_against_float64(ops, kind, rows, hub, min_octets, conj, full):
    """gradients of the rotated path against the float64 vector-ALU kernels at the tolerance of the existing pair tests (1e-4 of
    the largest entry), two runs bit-identical"""
    ant = _array(kind)
    Nt, Nf, P = 2, 5, 704
    pairs, blvecs, freqs, sdir, g = _inputs(ant, Nt, Nf, P, 17, full)
    geom = ops.FringeGeometry(blvecs, sdir, freqs, conj=conj, antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True)
    assert geom.ant is not None and geom.ant['pair_blocks'] == [((len(ant) - 1) // 2, rows, hub)], geom.ant['pair_blocks']
    blk = geom.ant['blocks_real'][0]
    assert blk['pair'] == 1 and (blk['centre'] is not None) == bool(hub)
    mask = ops._pair_ap_mask((blk['bwd'] or blk)['pos'].cpu().numpy())
    assert bin(mask).count('1') >= min_octets, bin(mask)
    ref_geom = ops.FringeGeometry(blvecs, sdir, freqs, conj=conj, mfma=False)
    ref = ops.fringe_adjoint(g, ref_geom)
    assert ref.dtype == torch.float64
    out = [ops.fringe_adjoint(g.to(torch.complex64), geom).clone() for _ in range(2)]
    assert torch.equal(out[0], out[1])
    err = float((out[0].double() - ref).abs().max() / ref.abs().max())
    print('%s conj=%d full=%d: mask %s, max |grad - float64| / max |grad| = %.2e' % (kind, conj, full, bin(mask), err))
    assert err < 1e-4


_AB_SCRIPT = r'''
import sys, zlib
import numpy as np, torch
sys.path.insert(0, %(root)r)
from bayeslim_amd import ops
rng = np.random.default_rng(23)
h = rng.normal(0, 70.0, (45, 3)) * [1, 1, 0.05]
ant = np.vstack([h, -h, rng.normal(0, 70.0, (10, 3)) * [1, 1, 0.05]])
ant = ant[rng.permutation(len(ant))] + [31.7, -12.3, 4.1]
n, Nt, Nf, P = len(ant), 2, 5, 704
pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
blvecs = T64(np.stack([ant[b] - ant[a] for a, b in pairs])).cuda()
s = rng.normal(size=(Nt, 3, P)); s /= np.linalg.norm(s, axis=1, keepdims=True); s[:, 2] = np.abs(s[:, 2])
g = torch.as_tensor(rng.normal(size=(1, len(pairs), Nt, Nf)) + 1j * rng.normal(size=(1, len(pairs), Nt, Nf))).to(torch.complex64).cuda()
geom = ops.FringeGeometry(blvecs, T64(s).cuda(), T64(np.linspace(120e6, 180e6, Nf)), antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True)
assert geom.ant['pair_blocks'] == [(45, 55, 0)], geom.ant['pair_blocks']
out = ops.fringe_adjoint(g, geom).cpu().numpy()
print('CRC', zlib.crc32(out.tobytes()), float(np.abs(out).max()))
'''


def test_switch_changes_nothing_without_progressions():
    """a seeded random point-symmetric array on the pair kernels: gradients bit-identical between RIME_PAIR_AP=1 and 0 (the switch
    is read once per process by the library: one fresh child process each)"""
    crc = {}
    for on in ('1', '0'):
        env = dict(os.environ, RIME_PAIR_AP=on)
        r = subprocess.run([sys.executable, '-c', _AB_SCRIPT % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        crc[on] = [ln for ln in r.stdout.splitlines() if ln.startswith('CRC')][0]
    assert crc['1'] == crc['0'], crc
