"""
Every matrix-core fringe kernel instantiation (tests/fringe_kernel_table.py) in the regime where the round-5 defect appeared:
launch grids of at least two blocks per CU times the kernel's minimum blocks per CU, so that most blocks are dispatched while
others stream MFMAs on the same CU (keep_scalar in csrc/fringe_mfma_common.h).

Each case builds one antenna array (random or point-symmetric, partial pair sets with autocorrelations, beam-model pairs,
groups of 32 / 64 / 128 antennas, real or complex psky, both fringe signs) on a pixel axis with a ragged tail, and checks

  * every visibility and every psky-gradient entry against the float64 baseline-formulation kernels (mfma=False, pinned to
    the oracle and the golden fixtures) on the same float32 inputs cast exactly to float64, normalised per block -- the
    largest error over one antenna block's baselines at one (t, f) over the largest |V| there (1e-5), per (t, f) psky row for
    the gradient (1e-4) -- so that one wrong block is not diluted by the others;
  * sampled float64 sums of the defining formula  V = sum_p psky exp(+-2 pi i nu/c b.s)  at the blocks dispatched last (last
    time, last channels, the last pixel split and the ragged tail), for the baselines of each antenna block's last rows (its
    padded row tile), which also catches a defect the two kernel families would share;
  * three runs of forward and backward: bit-identical.

A thin proxy in place of ops.lib records the arguments of every rime_fringe_ant_{fwd,bwd}_block and
rime_fringe_pair_{fwd,bwd}_block call and maps them through the table to instantiations: each case asserts that it
launched the rows the table assigns to it, and the last test that the cases together launched every row.
"""
import zlib

import numpy as np
import pytest
import torch

import fringe_kernel_table as kt
from fringe_kernel_table import CASES, LaunchRecorder, build_case

pytestmark = pytest.mark.gpu

C_LIGHT = 2.99792458e8
NT, NF = 3, 520                   # 1560 (t, f) rows: >= 2 x 256 CUs x 3 blocks per CU with one pixel split
TOL_VIS, TOL_GRAD = 1e-5, 1e-4

LAUNCHED = {}                     # table row -> case ids that launched it
WORST = {}                        # table row -> worst per-block ratio seen (vis for forward rows, gradient for backward)
CASES_RUN = set()


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def _sdir(Nt, P, Ps, gen):
    """random unit vectors of the visible hemisphere per time, zero past P"""
    s = torch.randn(Nt, 3, P, dtype=torch.float64, device='cuda', generator=gen)
    s /= s.norm(dim=1, keepdim=True)
    s[:, 2].abs_()
    out = torch.zeros(Nt, 3, Ps, dtype=torch.float64, device='cuda')
    out[..., :P] = s
    return out


def _psky(shape, P, cplx, gen):
    """beam-like psky (six decades of envelope) on the padded pixel axis; rows f = 1 mod 4 and the last row of every plane
    hold no negative value (the mask-free SIGNED = false instantiations; for a complex psky its real plane)"""
    def plane():
        f32 = dict(dtype=torch.float32, device='cuda', generator=gen)        # whatever torch's default dtype
        x = torch.randn(shape, **f32) * torch.exp(-9.0 * torch.rand(shape, **f32))
        x[:, :, :, 1::4] = x[:, :, :, 1::4].abs()
        x[-1, :, :, -1] = x[-1, :, :, -1].abs()
        x[..., P:] = 0
        return x
    return torch.complex(plane(), plane()) if cplx else plane()


def _block_baselines(blk):
    slots = [blk['direct'], blk['conj']] + ([blk['centre']] if blk.get('centre') is not None else [])
    return torch.cat([t[t >= 0] for t in slots]).to(torch.int64)


def _last_row_baselines(blk, k=6):
    """up to k baselines of the block's last rows (largest row index of its tables: its last, padded row tile) and, for a
    block with a hub, two of the hub's"""
    out = []
    for tab in (blk['direct'], blk['conj']):
        t = tab.reshape(128, 128)
        i, j = torch.nonzero(t >= 0, as_tuple=True)
        order = torch.argsort(torch.maximum(i, j), descending=True)[:k]
        out.append(t[i[order], j[order]])
    if blk.get('centre') is not None:
        c = blk['centre']
        out.append(c[c >= 0][-2:])
    return torch.cat(out).to(torch.int64).unique()[:2 * k + 2]


def _formula_vis(x, blvecs, sdir, freqs, sign, bsel, mp, t, f):
    """float64 sum of the defining formula for the baselines bsel at (t, f): (Npp, len(bsel))"""
    tau = blvecs[bsel] @ sdir[t]                                                        # (nb, Ps) metres
    ph = torch.exp((sign * 2j * np.pi / C_LIGHT * float(freqs[f])) * tau)
    xs = x[t, mp[bsel], :, f].to(torch.complex128)                                     # (nb, Npp, Ps)
    return (ph[:, None] * xs).sum(-1).T


def _formula_grad(G, blvecs, sdir, freqs, sign, bl_mp, plane, psel, t, f):
    """float64 psky gradient of Re sum V conj(G) at pixels psel of (t, plane, f): sum_b conj(F) G over the plane's baselines"""
    b = torch.nonzero(bl_mp == plane, as_tuple=True)[0]
    tau = blvecs[b] @ sdir[t][:, psel]                                                  # (nb, np)
    ph = torch.exp((sign * 2j * np.pi / C_LIGHT * float(freqs[f])) * tau)
    return (ph.conj()[None] * G[:, b, t, f].to(torch.complex128)[:, :, None]).sum(1)     # (Npp, np)


@pytest.mark.parametrize('cid', list(CASES))
def test_fringe_kernels_coresident_against_float64(ops, cid, monkeypatch):
    spec = CASES[cid]
    P = spec.get('P', 1000)
    assert P % 64, 'the pixel axis needs a ragged tail'
    Ps = ops.pad_to_tile(P)
    sign = -1 if spec.get('conj') else 1
    ant, pairs, bl_mp, mp_pairs = build_case(cid)
    Nbl, Nmp = len(pairs), (len(mp_pairs) if mp_pairs else 1)
    monkeypatch.setattr(ops, 'MIRROR', True)
    monkeypatch.setattr(ops, 'PAIR', spec.get('pair', True))
    monkeypatch.setattr(ops, 'PAIR_CPLX', True)
    monkeypatch.setattr(ops, 'SELF_BLOCKS', True)
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32(cid.encode()))
    antp = torch.as_tensor(ant, dtype=torch.float64, device='cuda')
    i1 = torch.as_tensor([a for a, _ in pairs], device='cuda')
    i2 = torch.as_tensor([b for _, b in pairs], device='cuda')
    blvecs = antp[i2] - antp[i1]
    sdir = _sdir(NT, P, Ps, gen)
    freqs = torch.linspace(120e6, 180e6, NF, dtype=torch.float64)
    kw = dict(bl_mp=bl_mp, Nmp=Nmp, conj=sign < 0)
    gm = ops.FringeGeometry(blvecs, sdir, freqs, antpos=antp, bl_ants=pairs, mfma=True, group=spec.get('group'),
                            mp_pairs=mp_pairs, **kw)
    gv = ops.FringeGeometry(blvecs, sdir, freqs, mfma=False, **kw)
    assert gm.ant is not None and gv.ant is None
    mp = torch.as_tensor(bl_mp if bl_mp else [0] * Nbl, device='cuda')
    fq = freqs.cuda()

    cu = torch.cuda.get_device_properties(0).multi_processor_count
    rec = LaunchRecorder(ops.lib)
    monkeypatch.setattr(ops, 'lib', rec)
    report, launched = {}, set()
    for kind in spec.get('psky', ('real',)):
        cplx = kind == 'complex'
        rec.calls.clear()
        x = _psky((NT, Nmp, 1, NF, Ps), P, cplx, gen)
        f32 = dict(dtype=torch.float32, device='cuda', generator=gen)
        G = torch.complex(torch.randn(1, Nbl, NT, NF, **f32), torch.randn(1, Nbl, NT, NF, **f32))
        runs = []
        for _ in range(3):
            xr = x.clone().requires_grad_(True)
            v = ops.fringe_sum(xr, gm)
            (g,) = torch.autograd.grad(v, xr, G)
            runs.append((v.detach(), g))
        nrec = len(rec.calls) // 3
        assert nrec and len(rec.calls) == 3 * nrec, (cid, x.dtype, len(rec.calls))
        del rec.calls[nrec:]                                                   # one run's launches
        rows = rec.rows()
        v, g = runs[0]
        for vv, gg in runs[1:]:
            assert torch.equal(vv, v) and torch.equal(gg, g), '%s %s: runs differ' % (cid, kind)

        # co-resident regime: every launch at least 2 x CUs x (the kernel's minimum blocks per CU)
        for row, entry, a in rows:
            blocks = kt.grid(entry, a['Nt'], a['Nf'], a['Pstride'])
            assert blocks >= 2 * cu * kt.KERNELS[row]['min_blocks'], (cid, row, blocks, cu)

        # float64 baseline-formulation kernels on the same float32 inputs
        x64 = x.to(torch.complex128 if cplx else torch.float64).requires_grad_(True)
        v64 = ops.fringe_sum(x64, gv)
        (g64,) = torch.autograd.grad(v64, x64, G.to(torch.complex128))
        v64, g64 = v64.detach(), g64.detach()

        # visibilities: per antenna block, per (t, f)
        blocks = gm.ant.get('blocks_cplx', gm.ant['blocks']) if cplx else gm.ant.get('blocks_real', gm.ant['blocks'])
        err = (v.to(torch.complex128) - v64).abs().amax(0)                    # (Nbl, Nt, Nf)
        mag = v64.abs().amax(0)
        seen = torch.zeros(Nbl, dtype=torch.bool, device='cuda')
        vis_ratio, samples = {}, []
        for blk in blocks:
            b = _block_baselines(blk)
            seen[b] = True
            r = float((err[b].amax(0) / mag[b].amax(0).clamp_min(1e-300)).max())
            vis_ratio[blk['direct'].data_ptr()] = r
            bs = _last_row_baselines(blk)
            for t, f in ((NT - 1, NF - 1), (NT - 1, NF - 2), (0, NF - 1)):
                ref = _formula_vis(x, blvecs, sdir, fq, sign, bs, mp, t, f)
                got = v[:, bs, t, f].to(torch.complex128)
                samples.append(float((got - ref).abs().max() / mag[b, t, f].max()))
        assert bool(seen.all()), 'every baseline belongs to a block'
        # gradient: per (t, plane, f) row over the valid pixels
        d = (g - g64)[..., :P].abs()
        grad_ratio = float((d.amax(-1) / g64[..., :P].abs().amax(-1).clamp_min(1e-300)).max())
        # the defining formula at the blocks dispatched last: last time and channel, the last pixel split of both
        # directions and the ragged tail
        S_f, S_b = kt.fwd_splits(NT, NF, Ps), kt.bwd_splits(NT, NF, Ps)
        starts = {(S_f - 1) * kt.fwd_split_pixels(NT, NF, Ps), (S_b[0] - 1) * S_b[1]}
        psel = sorted({p for s0 in starts for p in (s0, s0 + 1, (s0 + P) // 2)} | {P - 3, P - 2, P - 1})
        psel = torch.as_tensor([p for p in psel if p < P], device='cuda')
        gsamples = []
        for plane in range(Nmp):
            for t, f in ((NT - 1, NF - 1), (NT - 1, NF - 2)):
                ref = _formula_grad(G, blvecs, sdir, fq, sign, mp, plane, psel, t, f)
                got = g[t, plane, :, f][:, psel].to(torch.complex128)
                if not cplx:
                    ref = ref.real
                row = g64[t, plane, :, f, :P].abs().max()
                gsamples.append(float((got - ref).abs().max() / row))

        for row, entry, a in rows:
            launched.add(row)
            r = vis_ratio[a['direct']] if entry in (kt.FWD, kt.PFWD) else grad_ratio
            report[row] = max(report.get(row, 0.0), r)
        worst = '\n'.join('  %-48s %-13s %.2e' % (k[0], k[1], r) for k, r in sorted(report.items()))
        msg = '%s (%s psky): worst per-block ratio per instantiation\n%s' % (cid, kind, worst)
        assert max(vis_ratio.values()) < TOL_VIS, msg
        assert grad_ratio < TOL_GRAD, msg
        assert max(samples) < TOL_VIS, '%s: defining formula at the late blocks, vis %.2e\n%s' % (cid, max(samples), msg)
        assert max(gsamples) < TOL_GRAD, '%s: defining formula at the late blocks, grad %.2e\n%s' % (cid, max(gsamples), msg)
        del runs, v, g, v64, g64, x64, err, mag, d

    for row, r in report.items():
        LAUNCHED.setdefault(row, set()).add(cid)
        WORST[row] = max(WORST.get(row, 0.0), r)
    CASES_RUN.add(cid)
    mine = {row for row, info in kt.KERNELS.items() if info['case'] == cid}
    assert mine <= launched, '%s did not launch %s' % (cid, sorted(mine - launched))
    torch.cuda.empty_cache()


def test_every_table_row_was_launched():
    """after the cases above: the table's rows were all launched (the cases are the table's `case` column)"""
    assert {info['case'] for info in kt.KERNELS.values()} <= set(CASES)
    assert CASES_RUN == set(CASES), 'run the whole module: cases %s did not run' % sorted(set(CASES) - CASES_RUN)
    missing = sorted(set(kt.KERNELS) - set(LAUNCHED))
    print('\nworst per-block ratio per instantiation (vis: forward rows, gradient: backward rows)')
    for row in sorted(kt.KERNELS):
        print('  %-48s %-13s %.2e  %s' % (row[0], row[1], WORST.get(row, float('nan')), ','.join(sorted(LAUNCHED.get(row, ())))))
    assert not missing, 'table rows no case launched: %s' % missing
