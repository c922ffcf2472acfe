"""Child process of tests/test_fringe_segments_gpu.py (the package reads RIME_FRINGE_MERGE at import): runs every case of
CASES through ops.fringe_sum_components -- one merged launch per direction with the switch on, one launch sequence per sky
component with it off -- three times, holds the visibilities and the gradients to the bounds of the float64 vector-ALU
kernels, and writes the arrays of every case (argv[1]/<case>.npz) and one record per case (argv[1]/records.json)."""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import fringe_kernel_table as kt                     # noqa: E402

NT, NF = 2, 3
TOL_VIS, TOL_GRAD = 1e-5, 1e-4                       # tests/test_fringe_kernels_gpu.py: max-norm per (t, f), float64 kernels
# case -> array (hex127+1: 64 rows + hub, FLAT, two row tiles; hex37: one row tile), pixels per segment, sign kind per segment
# ('mixed': rows with negative values and rows without; 'pos': no negative value), segments whose psky requires a gradient
CASES = {
    'two-mixed-pos': ('hex127+1', (70, 33), ('mixed', 'pos'), (True, True)),
    'two-pos-mixed': ('hex127+1', (70, 33), ('pos', 'mixed'), (True, True)),
    'three': ('hex127+1', (1, 64, 95), ('mixed', 'pos', 'mixed'), (True, True, True)),
    'one-tile': ('hex37', (70, 33), ('mixed', 'pos'), (True, True)),
    'one-tile-three': ('hex37', (1, 64, 95), ('pos', 'mixed', 'mixed'), (True, True, True)),
    'first-splits': ('hex127+1', (16400, 33), ('mixed', 'pos'), (True, True)),
    'later-splits': ('hex127+1', (70, 2100), ('mixed', 'mixed'), (True, True)),
    'no-grad': ('hex127+1', (70, 33), ('mixed', 'pos'), (True, False)),
    'no-grad-first': ('hex37', (70, 33), ('mixed', 'pos'), (False, True)),
}


class Recorder:
    """stands in for ops.lib: forwards every call and records the names of the fringe entry points called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('rime_fringe_') or name.endswith('_workspace'):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def build_array(kind, rng):
    pos = kt._positions(kind, rng)
    n = len(pos)
    hub = int(np.argmin(np.abs(pos - pos.mean(0)).sum(1))) if '+1' in kind else None
    pairs = [(i, j) if rng.random() < 0.5 else (j, i) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.8]
    pairs += [(a, a) for a in range(0, n, 17) if a != hub][:3]
    return pos, [pairs[k] for k in rng.permutation(len(pairs))]


def ratios(v, v64, grads, g64s, Ps):
    err = (v.to(torch.complex128) - v64).abs().amax((0, 1))                       # (Nt, Nf)
    rv = float((err / v64.abs().amax((0, 1)).clamp_min(1e-300)).max())
    rg = 0.0
    for g, g64, P in zip(grads, g64s, Ps):
        if g is not None:
            d = (g.to(torch.float64) - g64)[..., :P].abs().amax(-1)
            rg = max(rg, float((d / g64[..., :P].abs().amax(-1).clamp_min(1e-300)).max()))
    return rv, rg


def run_case(ops, name, outdir):
    import test_fringe_kernels_gpu as base
    kind, pixels, signs, needs = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32(name.encode()))
    ant, pairs = build_array(kind, rng)
    Nbl = len(pairs)
    antp = torch.as_tensor(ant, dtype=torch.float64, device='cuda')
    i1 = torch.as_tensor([a for a, _ in pairs], device='cuda')
    i2 = torch.as_tensor([b for _, b in pairs], device='cuda')
    blvecs = antp[i2] - antp[i1]
    freqs = torch.linspace(120e6, 180e6, NF, dtype=torch.float64)
    geoms, g64s, xs = [], [], []
    for P, sk in zip(pixels, signs):
        Ps = ops.pad_to_tile(P)
        sdir = base._sdir(NT, P, Ps, gen)
        geoms.append(ops.FringeGeometry(blvecs, sdir, freqs, antpos=antp, bl_ants=pairs, mfma=True,
                                        ant_like=geoms[0] if geoms else None))
        g64s.append(ops.FringeGeometry(blvecs, sdir, freqs, mfma=False))
        x = base._psky((NT, 1, 1, NF, Ps), P, False, gen)
        if sk == 'pos':
            x = x.abs()
        else:
            x[:, :, :, 1] = x[:, :, :, 1].abs()                                   # one row of a mixed segment without a sign
            x[:, :, :, 0, 0] = -x[:, :, :, 0, 0].abs() - 1e-3                      # ... and one with, whatever the draw
        xs.append(x)
    blk = geoms[0].ant['blocks_real'][0]
    assert blk.get('pair') and all(g.ant['blocks_real'][0] is blk for g in geoms)
    f32 = dict(dtype=torch.float32, device='cuda', generator=gen)
    G = torch.complex(torch.randn(1, Nbl, NT, NF, **f32), torch.randn(1, Nbl, NT, NF, **f32))

    rec = Recorder(ops.lib)
    real_lib, ops.lib = ops.lib, rec
    try:
        runs = []
        for _ in range(3):
            xr = [x.clone().requires_grad_(n) for x, n in zip(xs, needs)]
            v = ops.fringe_sum_components(xr, geoms)
            gs = torch.autograd.grad(v, [x for x, n in zip(xr, needs) if n], G)
            it = iter(gs)
            runs.append((v.detach(), [next(it) if n else None for n in needs]))
    finally:
        ops.lib = real_lib
    v, grads = runs[0]
    for w, hs in runs[1:]:
        assert torch.equal(v, w), '%s: visibilities differ between runs' % name
        assert all(g is None or torch.equal(g, h) for g, h in zip(grads, hs)), '%s: gradients differ between runs' % name
    entries = rec.calls

    x64 = [x.double().requires_grad_(True) for x in xs]
    v64 = sum(ops.fringe_sum(x, g) for x, g in zip(x64, g64s))
    ref = torch.autograd.grad(v64, x64, G.to(torch.complex128))
    rv, rg = ratios(v, v64.detach(), grads, ref, pixels)
    print('%-16s vis %.2e  grad %.2e' % (name, rv, rg), flush=True)
    assert rv < TOL_VIS, '%s: visibilities against float64 %.2e' % (name, rv)
    assert rg < TOL_GRAD, '%s: gradients against float64 %.2e' % (name, rg)

    arrays = dict(vis=torch.view_as_real(v).cpu().numpy())
    for k, g in enumerate(grads):
        if g is not None:
            arrays['grad%d' % k] = g.cpu().numpy()
    record = dict(vis=rv, grad=rg, entries=sorted(set(entries)), calls=len(entries) // 3)

    if name in ('two-mixed-pos', 'one-tile'):
        # one segment through the segment entry points against the single-plane entry points
        xr = xs[0].clone().requires_grad_(True)
        vo = ops.fringe_sum(xr, geoms[0])
        (go,) = torch.autograd.grad(vo, xr, G)
        vn = torch.empty_like(vo)
        gn = torch.empty_like(go)
        ops._merged_call(blk, geoms[:1], False, [xs[0]], torch.view_as_real(vn))
        ops._merged_call(blk, geoms[:1], True, [gn], torch.view_as_real(G.contiguous()))
        record['single'] = bool(torch.equal(vo.detach(), vn) and torch.equal(go, gn))
    np.savez(os.path.join(outdir, name + '.npz'), **arrays)
    return record


def main(outdir):
    assert torch.cuda.is_available()
    from bayeslim_amd import ops
    ops.MIRROR, ops.PAIR = True, True
    res = {'merge': bool(ops.FRINGE_MERGE)}
    for name in CASES:
        res[name] = run_case(ops, name, outdir)
    with open(os.path.join(outdir, 'records.json'), 'w') as f:
        json.dump(res, f)


if __name__ == '__main__':
    main(sys.argv[1])
