"""
Every vector-ALU fringe kernel instantiation of csrc/fringe.hip (tests/fringe_valu_table.py) against the float64 CPU oracle
(oracle/rime_oracle.py: the defining formula, not another kernel).

Each case of the table runs ops.fringe_sum and its autograd backward (ops.fringe_adjoint / ops.gen_fringe where the case
says so) under a recorder in place of ops.lib, asserts that the launched kernels are the rows the case states, and compares
ALL visibilities and ALL psky-gradient entries with the oracle on the same inputs (float32 psky cast exactly):

  * visibilities: the largest error over the baselines of one (plane, model pair, t, f) row over the largest |V| of that row;
  * gradient: the largest error over the valid pixels of one (t, model pair, plane, f) psky row over the largest |g| there;
    padded columns finite; the plane of a model pair without baselines exactly zero.

Bounds are the project's: float64 1e-11 (1e-10 on km baselines), float32 1e-5 for visibilities and 1e-4 for gradients.
The cases cover every (T, NPP, CPLX) x MODE row in both directions -- the shear modes at 0.29 turn per channel, the 0.3-turn
switch from both sides, near-uniform grids up to phi = 1.9e-3 -- and the edges of the launch plans (see CASES).
"""
import numpy as np
import pytest
import torch

import fringe_valu_table as vt
from fringe_valu_table import CASES, LaunchRecorder, build_case
from oracle import rime_oracle as orc

pytestmark = pytest.mark.gpu

T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)

LAUNCHED = {}                     # table row -> case ids that launched it
WORST = {}                        # table row -> worst ratio seen (visibilities for forward rows, gradient for backward rows)
CASES_RUN = set()


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def _oracle(c, spec, want_vis=True):
    """float64 visibilities (Npp, Nbl, Nt, Nf) and psky gradient of Re sum V conj(G), (Nt, Nmp, Npp, Nf, P), from the
    oracle's fringe, in chunks of baselines"""
    blv, fr, za = T64(c['blvecs']), T64(c['freqs']), T64(c['zenaz'])
    psky, G = torch.as_tensor(c['psky']), torch.as_tensor(c['gvis'])
    mp = torch.as_tensor(c['bl_mp'])
    Nt, Nmp, Npp, Nf, P = psky.shape
    V = torch.zeros((Npp, c['Nbl'], Nt, Nf), dtype=torch.complex128)
    gp = torch.zeros(psky.shape, dtype=torch.complex128)
    nb = max(1, int(1e7 // (Nf * P * Npp)))
    for t in range(Nt):
        for b0 in range(0, c['Nbl'], nb):
            sl = slice(b0, min(b0 + nb, c['Nbl']))
            F = orc.gen_fringe(blv[sl], za[t, 0], za[t, 1], fr, conj=spec['conj'])            # (nb, Nf, P)
            if want_vis:
                V[:, sl, t] = torch.einsum('bfp,bqfp->qbf', F, psky[t][mp[sl]].to(torch.complex128))
            gp[t].index_add_(0, mp[sl], F.conj()[:, None] * G[:, sl, t].permute(1, 0, 2)[..., None])
    return V, (gp if c['cplx'] else gp.real)


def _vis_ratio(v, ref, bl_mp, Nmp):
    """largest error over one model pair's baselines at one (plane, t, f) over the largest |V| there; the worst row"""
    err, mag = (v - ref).abs(), ref.abs()
    worst = 0.0
    for m in range(Nmp):
        b = np.nonzero(bl_mp == m)[0]
        if len(b):
            r = err[:, b].amax(1) / mag[:, b].amax(1).clamp_min(1e-300)
            worst = max(worst, float(r.max()))
    return worst


def _grad_ratio(g, ref):
    """largest error over the pixels of one (t, model pair, plane, f) row over the largest |g| of the row; rows the oracle
    holds no gradient for (a model pair without baselines) are compared exactly elsewhere"""
    err, mag = (g - ref).abs().amax(-1), ref.abs().amax(-1)
    keep = mag > 0
    return float((err[keep] / mag[keep]).max()) if bool(keep.any()) else 0.0


@pytest.mark.parametrize('cid', list(CASES))
def test_fringe_valu_kernels_against_the_oracle(ops, cid, monkeypatch):
    spec = CASES[cid]
    c = build_case(cid)
    f64 = spec['dtype'] == 'f64'
    rdt, cdt = (torch.float64, torch.complex128) if f64 else (torch.float32, torch.complex64)
    tol_v, tol_g = ((1e-10, 1e-10) if spec.get('km') else (1e-11, 1e-11)) if f64 else (1e-5, 1e-4)
    Nt, Nf, P, Nmp, Npp, cplx = spec['Nt'], spec['Nf'], spec['P'], c['Nmp'], c['Npp'], c['cplx']
    Ps = ops.pad_to_tile(P)
    za = T64(c['zenaz'])
    sdir = torch.zeros(Nt, 3, Ps, dtype=torch.float64)
    for t in range(Nt):
        sdir[t, :, :P] = orc.pointing_vectors(za[t, 0], za[t, 1])
    rec = LaunchRecorder(ops.lib)
    monkeypatch.setattr(ops, 'lib', rec)
    vis_ratio = grad_ratio = None

    if spec.get('gen'):
        got = ops.gen_fringe(T64(c['blvecs']).cuda(), sdir[0, :, :P].cuda(), c['freqs'], conj=spec['conj'], dtype=rdt)
        ref = orc.gen_fringe(T64(c['blvecs']), za[0, 0], za[0, 1], T64(c['freqs']), conj=spec['conj'])
        assert got.shape == ref.shape and got.dtype == cdt
        vis_ratio = float((got.cpu().to(torch.complex128) - ref).abs().amax((0, 2)).max())      # |F| = 1: per channel
    else:
        geom = ops.FringeGeometry(T64(c['blvecs']).cuda(), sdir.cuda(), c['freqs'], bl_mp=c['bl_mp'], Nmp=Nmp,
                                  conj=spec['conj'])
        # the case is what it says: grid kind, step per channel, phase residual
        assert geom.uniform == {'uniform': 1, 'near': 2, 'ragged': 0}[spec['grid']], (cid, geom.uniform)
        if spec['step'] is not None:
            step = geom.max_blen * geom.df / vt.C_LIGHT
            assert abs(abs(step) - spec['step']) < 1e-6 * spec['step'] and (step < 0) == (spec['df'] < 0), (cid, step)
        if spec['grid'] == 'near':
            assert abs(geom.nu_phi / spec['phi'] - 1) < 1e-3, (cid, geom.nu_phi)
        assert (geom.bl_order is not None) == (Nmp > 1)
        G = torch.as_tensor(c['gvis']).to(cdt).cuda()
        V64, g64 = _oracle(c, spec, want_vis=not spec.get('adjoint'))
        if spec.get('adjoint'):
            g = ops.fringe_adjoint(G, geom)
            assert g.shape == (Nt, 1, Npp, Nf, Ps) and g.dtype == rdt
            runs = [(None, g)]
        else:
            pad = torch.zeros(c['psky'].shape[:-1] + (Ps,), dtype=cdt if cplx else rdt)
            pad[..., :P] = torch.as_tensor(c['psky']).to(pad.dtype)
            runs = []
            for _ in range(spec.get('repeat', 1)):
                if spec.get('strided'):                      # time-inner (Npp, Nmp, Nf, Nt, Ps) storage, permuted view
                    leaf = pad.permute(2, 1, 3, 0, 4).contiguous().cuda().requires_grad_(True)
                    x = leaf.permute(3, 1, 0, 2, 4)
                    assert not x.is_contiguous()
                else:
                    leaf = x = pad.cuda().requires_grad_(True)
                v = ops.fringe_sum(x, geom)
                assert v.shape == (Npp, c['Nbl'], Nt, Nf) and v.dtype == cdt
                (g,) = torch.autograd.grad(v, leaf, G)
                runs.append((v.detach(), g.permute(3, 1, 0, 2, 4) if spec.get('strided') else g))
            for vv, gg in runs[1:]:
                assert torch.equal(vv, runs[0][0]) and torch.equal(gg, runs[0][1]), '%s: runs differ' % cid
            n = len(rec.calls) // len(runs)
            del rec.calls[n:]                                  # one run's launches
        v, g = runs[0]
        g = g.cpu()
        assert bool(torch.isfinite(g).all()), '%s: gradient not finite (padded columns included)' % cid
        empty = [m for m, n in enumerate(spec['groups']) if n == 0]
        for m in empty:                                        # no baseline: the whole plane exactly zero
            assert int(torch.count_nonzero(g[:, m])) == 0, '%s: gradient plane %d of a pair without baselines' % (cid, m)
            assert int(torch.count_nonzero(g64[:, m])) == 0
        ctype = torch.complex128 if cplx else torch.float64
        grad_ratio = _grad_ratio(g[..., :P].to(ctype), g64)
        if v is not None:
            vis_ratio = _vis_ratio(v.cpu().to(torch.complex128), V64, c['bl_mp'], Nmp)

    rows = {row for row, _, _ in rec.rows()}
    print('\n%s: vis %s grad %s | %s' % (cid, '-' if vis_ratio is None else '%.2e' % vis_ratio,
                                        '-' if grad_ratio is None else '%.2e' % grad_ratio, ', '.join(sorted(rows))))
    assert rows == vt.expected_rows(cid), (cid, sorted(rows ^ vt.expected_rows(cid)))
    for row in rows:
        fwd = vt.KERNELS[row]['entry'] != vt.SBWD
        r = vis_ratio if fwd else grad_ratio
        LAUNCHED.setdefault(row, set()).add(cid)
        WORST[row] = max(WORST.get(row, 0.0), r)
    CASES_RUN.add(cid)
    if vis_ratio is not None:
        assert vis_ratio < tol_v, '%s: visibilities %.2e (bound %.0e)' % (cid, vis_ratio, tol_v)
    if grad_ratio is not None:
        assert grad_ratio < tol_g, '%s: psky gradient %.2e (bound %.0e)' % (cid, grad_ratio, tol_g)
    torch.cuda.empty_cache()


def test_every_table_row_was_launched():
    """after the cases above: the table's rows were all launched (the cases are the table's `case` column)"""
    assert {info['case'] for info in vt.KERNELS.values()} <= set(CASES)
    assert CASES_RUN == set(CASES), 'run the whole module: cases %s did not run' % sorted(set(CASES) - CASES_RUN)
    print('\nworst ratio per kernel (visibilities: forward rows, gradient: backward rows), cases that launched it')
    for row in sorted(vt.KERNELS):
        cases = sorted(LAUNCHED.get(row, ()))
        print('  %-52s %.2e  %d: %s' % (row, WORST.get(row, float('nan')), len(cases), ','.join(cases[:4])))
    print('worst ratio per type, direction and mode')
    names = {v: k for k, v in vt.MODES.items()}
    summary = {}
    for row, r in WORST.items():
        if row.startswith('fringe_'):
            p = row[row.index('<') + 1:-1].split(', ')
            key = (p[0], row[7:10], names[int(p[4])])
            summary[key] = max(summary.get(key, 0.0), r)
    for key in sorted(summary):
        print('  %-6s %s %-8s %.2e' % (key + (summary[key],)))
    missing = sorted(set(vt.KERNELS) - set(LAUNCHED))
    assert not missing, 'table rows no case launched: %s' % missing
