"""
RIME.forward and its gradients on a hex-169 (14 196 baselines) against outputs of the imported reference
(tests/golden/rime_hex169_mini.npz, written by tests/golden/make_golden_hex169.py), at the tolerances
test_rime_matrix_core_arrays_against_reference applies to the headline array; in float32 the pair cross plan must be the one taken.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_rime_gpu import T, _c2_setup, _profiled, ba, prec, relmax, tols  # noqa: F401  (ba, prec: fixtures)

pytestmark = pytest.mark.gpu


def test_rime_hex169_against_reference(ba, prec):
    from bayeslim_amd import ops
    g = load_golden('rime_hex169_mini')
    gvis = (g['gvis_re_i8'].astype(np.float64) + 1j * g['gvis_im_i8'].astype(np.float64)) / 64.0     # exact (see the generator)
    rime, sky, beam = _c2_setup(ba, g)
    tv, tg = tols(prec)

    def run():
        vd = rime()
        loss = (vd.data * T(gvis).conj()).real.sum()
        return vd.data, torch.autograd.grad(loss, [sky.params, beam.params])

    (vis, grads), kernels = _profiled(ops, run)
    assert vis.shape == (1, 1, 14196, 2, len(g['freqs']))
    if prec == 'f32':
        assert kernels == ['fringe_ant_fwd_kernel', 'fringe_ant_bwd_kernel'], kernels
        assert ops.PAIR_CROSS and ops.MIRROR and ops.PAIR
        ants = [bg['geom'].ant for bg in rime._geom_cache.values() if bg['geom'].ant is not None]
        assert ants and all(a.get('pair_cross_blocks') == [(43, 42)] and a['pair_blocks'] == [(43, 43, 0), (41, 42, 0)] for a in ants), \
            [(a.get('pair_cross_blocks'), a.get('pair_blocks')) for a in ants]
        assert all(any(b.get('xpair') for b in a['blocks_real']) for a in ants)
    assert relmax(vis, g['vis']) < tv
    if prec == 'f32':
        # element by element, as for the headline array: the error relative to each visibility itself
        v = vis.detach().cpu().numpy().astype(np.complex128)
        e = np.abs(v - g['vis']) / np.abs(g['vis'])
        print('hex169 f32: max-norm %.2e, elementwise median %.2e, 99th percentile %.2e' % (relmax(vis, g['vis']), np.median(e), np.quantile(e, 0.99)))
        assert np.median(e) < 2e-6 and np.quantile(e, 0.99) < 1e-5, (np.median(e), np.quantile(e, 0.99))
        big = np.abs(g['vis']) > 0.05 * np.abs(g['vis']).max()
        assert e[big].max() < 1e-5, e[big].max()
    for gr, n in zip(grads, ['g_sky_params', 'g_beam_params']):
        assert relmax(gr, g[n]) < tg, n
