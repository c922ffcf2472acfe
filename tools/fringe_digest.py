#!/usr/bin/env python3
"""
One CRC32 per case of the matrix-core fringe kernels' outputs: the forward visibilities and the backward psky gradient.

Covers every case of tests/fringe_kernel_table.CASES (arrays and baselines from its build_case, the psky kinds the case names)
and every array of tests/pair_cross_cases.py (its make_array / make_pairs: the full pair set with the fringe sign +, the 90 %
subset with the sign -), on inputs seeded by the case id.  The library is whichever RIME_LIB_PATH names (bayeslim_amd/_lib.py), so two builds are
compared by

    RIME_LIB_PATH=/path/to/old/librime_hip.so python tools/fringe_digest.py > old.txt
    python tools/fringe_digest.py > new.txt && diff old.txt new.txt

A kernel change that claims the same arithmetic must leave every line as it was.  Arguments, if any, are substrings of the
case names to run.  Needs the GPU; not a test.
"""
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import fringe_kernel_table as kt          # noqa: E402
import pair_cross_cases as pc             # noqa: E402
from bayeslim_amd import ops              # noqa: E402

NT, NF = 2, 96


def crc(t):
    return zlib.crc32(t.detach().contiguous().cpu().numpy().tobytes())


def inputs(seed, Nt, Nmp, Nf, P, Ps, Nbl, cplx):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    f32 = dict(dtype=torch.float32, device='cuda', generator=gen)
    s = torch.randn(Nt, 3, P, dtype=torch.float64, device='cuda', generator=gen)
    s /= s.norm(dim=1, keepdim=True)
    s[:, 2].abs_()
    sdir = torch.zeros(Nt, 3, Ps, dtype=torch.float64, device='cuda')
    sdir[..., :P] = s

    def plane():
        shape = (Nt, Nmp, 1, Nf, Ps)
        x = torch.randn(shape, **f32) * torch.exp(-9.0 * torch.rand(shape, **f32))
        x[:, :, :, 1::4] = x[:, :, :, 1::4].abs()        # rows without a negative value: the mask-free instantiations
        x[..., P:] = 0
        return x
    x = torch.complex(plane(), plane()) if cplx else plane()
    G = torch.complex(torch.randn(1, Nbl, Nt, Nf, **f32), torch.randn(1, Nbl, Nt, Nf, **f32))
    return sdir, x, G


def digest(name, ant, pairs, P, conj, kinds=('real',), **geom_kw):
    if sys.argv[1:] and not any(a in name for a in sys.argv[1:]):
        return
    Ps = ops.pad_to_tile(P)
    antp = torch.as_tensor(np.asarray(ant), dtype=torch.float64, device='cuda')
    i1 = torch.as_tensor([a for a, _ in pairs], device='cuda')
    i2 = torch.as_tensor([b for _, b in pairs], device='cuda')
    freqs = torch.linspace(120e6, 180e6, NF, dtype=torch.float64)
    Nmp = geom_kw.get('Nmp', 1)
    for kind in kinds:
        sdir, x, G = inputs(zlib.crc32(('%s %s' % (name, kind)).encode()), NT, Nmp, NF, P, Ps, len(pairs), kind == 'complex')
        geom = ops.FringeGeometry(antp[i2] - antp[i1], sdir, freqs, antpos=antp, bl_ants=pairs, mfma=True, conj=conj, **geom_kw)
        assert geom.ant is not None, name
        xr = x.requires_grad_(True)
        v = ops.fringe_sum(xr, geom)
        (g,) = torch.autograd.grad(v, xr, G)
        torch.cuda.synchronize()
        print('%-44s %-7s fwd %08x bwd %08x' % (name, kind, crc(v), crc(g)), flush=True)


def main():
    assert torch.cuda.is_available(), 'the digests are of GPU results'
    ops.MIRROR, ops.PAIR_CPLX, ops.SELF_BLOCKS = True, True, True
    for cid, spec in kt.CASES.items():
        ant, pairs, bl_mp, mp_pairs = kt.build_case(cid)
        ops.PAIR = spec.get('pair', True)
        digest(cid, ant, pairs, spec.get('P', 1000), bool(spec.get('conj')), spec.get('psky', ('real',)),
               group=spec.get('group'), mp_pairs=mp_pairs, bl_mp=bl_mp, Nmp=len(mp_pairs) if mp_pairs else 1)
    ops.PAIR = True
    for kind in pc.EXPECTED:
        for full in (True, False):
            rng = np.random.default_rng(pc.seed_of(kind, 7))
            ant = pc.make_array(kind, rng)
            pairs = pc.make_pairs(len(ant), rng, full)
            digest('cross:%s:%s' % (kind, 'full' if full else 'subset'), ant, pairs, 700, not full)


if __name__ == '__main__':
    main()
