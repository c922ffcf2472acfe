"""Child process of tests/test_pair_bwd_wide_gpu.py (the library reads RIME_PAIR_BWD_WIDE once): runs the pair backward of
every case at a shape whose launch plan widens, three times, checks the runs against each other and sampled (t, f) rows
against the float64 baseline-formulation kernels, and writes one record per case -- a digest of the gradient's bytes, the
splits the library reports, the instantiations launched -- as JSON to argv[1]."""
import hashlib
import json
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import fringe_kernel_table as kt                     # noqa: E402
from test_pair_bwd_split_host import pair_bwd_splits  # noqa: E402

# 3072 (t, f) rows x 1026 pixel tiles (the last one ragged): 5 splits of 256 tiles on the generic plan (15 360 blocks), 2 of
# 1024 on the widened one (6144 blocks: 8 per CU at 3 blocks per CU -- the co-resident regime of keep_scalar); the second
# split holds 2 tiles, so two of its four waves run no tile at all
NT, NF, P = 2, 1536, 32800
FSEL = [0, 777, NF - 1]
TOL_GRAD = 1e-4                                      # tests/test_fringe_kernels_gpu.py: per (t, f) row, float64 kernels
# two groups each: the first block writes its plane (accumulate 0), the second adds to it (accumulate 1); partial pair sets
# in random orientations (-1 entries and conjugated slots in the tables)
#   hex127+1 | hex37:   64 rows + hub, FLAT, progressions (two row tiles); hex37: one row tile
#   hex127+1t | sym45:  the same hexagon tilted (not FLAT); random mirror pairs and singles: no progression, one row tile
CASES = [(cid, kind) for cid in ('hex127+1+hex37', 'hex127+1t+sym45') for kind in ('real', 'complex')]


def run_case(ops, cid, kind):
    import test_fringe_kernels_gpu as base
    spec = kt.CASES[cid]
    Ps = ops.pad_to_tile(P)
    sign = -1 if spec.get('conj') else 1
    ant, pairs, _, _ = kt.build_case(cid)
    Nbl = len(pairs)
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32((cid + kind).encode()))
    antp = torch.as_tensor(ant, dtype=torch.float64, device='cuda')
    i1 = torch.as_tensor([a for a, _ in pairs], device='cuda')
    i2 = torch.as_tensor([b for _, b in pairs], device='cuda')
    blvecs = antp[i2] - antp[i1]
    sdir = base._sdir(NT, P, Ps, gen)
    freqs = torch.linspace(120e6, 180e6, NF, dtype=torch.float64)
    kw = dict(bl_mp=None, Nmp=1, conj=sign < 0)
    gm = ops.FringeGeometry(blvecs, sdir, freqs, antpos=antp, bl_ants=pairs, mfma=True, group=None, mp_pairs=None, **kw)
    gv = ops.FringeGeometry(blvecs, sdir, freqs[FSEL], mfma=False, **kw)
    assert gm.ant is not None and gv.ant is None
    cplx = kind == 'complex'
    x = base._psky((NT, 1, 1, NF, Ps), P, cplx, gen)
    f32 = dict(dtype=torch.float32, device='cuda', generator=gen)
    G = torch.complex(torch.randn(1, Nbl, NT, NF, **f32), torch.randn(1, Nbl, NT, NF, **f32))

    rec = kt.LaunchRecorder(ops.lib)
    real_lib, ops.lib = ops.lib, rec
    try:
        grads = []
        for _ in range(3):
            xr = x.clone().requires_grad_(True)
            v = ops.fringe_sum(xr, gm)
            (g,) = torch.autograd.grad(v, xr, G)
            grads.append(g)
            del v, xr
    finally:
        ops.lib = real_lib
    g = grads[0]
    assert all(torch.equal(g, h) for h in grads[1:]), '%s %s: three runs differ' % (cid, kind)
    del grads
    bwd = [(row, a) for row, entry, a in rec.rows() if entry == kt.PBWD]
    assert bwd and all(a['Nt'] == NT and a['Nf'] == NF and a['Pstride'] == Ps for _, a in bwd)

    # float64 kernels on the sampled channels (the gradient is linear in G and does not depend on psky)
    x64 = torch.zeros((NT, 1, 1, len(FSEL), Ps), dtype=torch.complex128 if cplx else torch.float64, device='cuda',
                      requires_grad=True)
    v64 = ops.fringe_sum(x64, gv)
    (g64,) = torch.autograd.grad(v64, x64, G[..., FSEL].to(torch.complex128))
    d = (g[:, :, :, FSEL] - g64)[..., :P].abs()
    ratio = float((d.amax(-1) / g64[..., :P].abs().amax(-1).clamp_min(1e-300)).max())
    assert ratio < TOL_GRAD, '%s %s: gradient against float64 %.2e' % (cid, kind, ratio)

    buf = torch.view_as_real(g).contiguous() if cplx else g.contiguous()
    digest = hashlib.blake2b(buf.cpu().numpy().tobytes(), digest_size=32).hexdigest()
    return dict(digest=digest, ratio=ratio, gmax=float(g.abs().max()), nbytes=buf.numel() * 4,
                splits=int(real_lib.rime_fringe_pair_bwd_splits(NT, NF, Ps)),
                generic=kt.bwd_splits(NT, NF, Ps)[0], wide=pair_bwd_splits(NT, NF, Ps)[0],
                launched=sorted({'%s %s' % row for row, _ in bwd}))


def main(out):
    assert torch.cuda.is_available()
    from bayeslim_amd import ops
    ops.MIRROR, ops.PAIR, ops.PAIR_CPLX, ops.SELF_BLOCKS = True, True, True, True
    res = {}
    for cid, kind in CASES:
        res['%s|%s' % (cid, kind)] = run_case(ops, cid, kind)
        torch.cuda.empty_cache()
    with open(out, 'w') as f:
        json.dump(res, f)


if __name__ == '__main__':
    main(sys.argv[1])
