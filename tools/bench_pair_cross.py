"""
Pair cross blocks against the parent commit: forward + backward fringe sum, float32, full pair sets of hex-169 and hex-217,
98 304 directions, 64 channels, 4 times.

One call on one box.  Every measurement is a child process of its own (one geometry, a warm-up, timed iterations between
device events); the configurations alternate round by round so that drift of the box hits all of them alike:
    parent   the parent commit's package and library (--parent-tree: a checkout of it with its library built), today's plan
    new on   this tree, RIME_PAIR_CROSS=1
    new off  this tree, RIME_PAIR_CROSS=0 (the old plan must not have moved)
Reported: the median over the rounds of each child's median, and the spread (max - min) over the rounds.

usage: python tools/bench_pair_cross.py --parent-tree DIR [--rounds 5] [--iters 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ARRAYS = {'hex169': 8, 'hex217': 9}


def child(args):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    import torch
    from bayeslim_amd import ops, utils
    T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    out = {}
    for kind in args.arrays.split(','):
        ant = utils._make_hex(ARRAYS[kind], D=14.6)[1]
        n, Nt, Nf, P = len(ant), args.nt, args.nf, args.npix
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        rng = np.random.default_rng(0)
        blvecs = T64(ant[[b for _, b in pairs]] - ant[[a for a, _ in pairs]]).cuda()
        freqs = T64(np.linspace(120e6, 180e6, Nf))
        s = rng.normal(size=(Nt, 3, P))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        s[:, 2] = np.abs(s[:, 2])
        sdir = T64(s).cuda()
        g = torch.as_tensor(rng.normal(size=(1, len(pairs), Nt, Nf)) + 1j * rng.normal(size=(1, len(pairs), Nt, Nf))).to(torch.complex64).cuda()
        psky = torch.as_tensor(rng.normal(size=(Nt, 1, 1, Nf, P))).float().cuda()
        geom = ops.FringeGeometry(blvecs, sdir, freqs, antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True)
        res = dict(nant=n, nbl=len(pairs), pair_cross_blocks=geom.ant.get('pair_cross_blocks'), pair_blocks=geom.ant.get('pair_blocks'),
                   mfma_fwd=geom.ant['mfma_fwd'], mfma_bwd=geom.ant['mfma_bwd'])
        for name, fn in (('fwd', lambda: ops.fringe_sum(psky, geom)), ('bwd', lambda: ops.fringe_adjoint(g, geom))):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            res[name + '_ms'] = float(np.median(ts))
            res[name + '_ms_all'] = [round(float(x), 3) for x in ts]
        out[kind] = res
    print('RESULT ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--arrays', default='hex169,hex217')
    ap.add_argument('--npix', type=int, default=98304)
    ap.add_argument('--nf', type=int, default=64)
    ap.add_argument('--nt', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import numpy as np
    configs = [('new on', ROOT, '1'), ('new off', ROOT, '0')]
    if args.parent_tree:
        configs.insert(0, ('parent', os.path.abspath(args.parent_tree), None))
    runs = {name: [] for name, _, _ in configs}
    for rnd in range(args.rounds):
        for name, tree, switch in configs:
            env = dict(os.environ)
            env.pop('RIME_LIB_PATH', None)
            env.pop('RIME_PAIR_CROSS', None)
            if switch is not None:
                env['RIME_PAIR_CROSS'] = switch
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--iters', str(args.iters), '--warmup', str(args.warmup),
                   '--arrays', args.arrays, '--npix', str(args.npix), '--nf', str(args.nf), '--nt', str(args.nt)]
            r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit('%s failed with status %d: no further measurement' % (name, r.returncode))
            line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1]
            runs[name].append(json.loads(line[7:]))
            print('round %d %-8s %s' % (rnd, name, {k: (round(v['fwd_ms'], 2), round(v['bwd_ms'], 2)) for k, v in runs[name][-1].items()}), flush=True)
    lines = ['pair cross blocks: fringe sum forward / backward, float32, full pair set, %d directions, %d channels, %d times' % (args.npix, args.nf, args.nt),
             'times MEASURED: median over %d alternating rounds of the median of %d iterations [ms], spread = max - min over the rounds;' % (args.rounds, args.iters),
             'MFMAs per 16-pixel K step DERIVED (geom.ant)', '']
    for kind in args.arrays.split(','):
        first = runs['new on'][0][kind]
        lines.append('%s (%d antennas, %d baselines): pair blocks %s, pair cross blocks %s' % (
            kind, first['nant'], first['nbl'], first['pair_blocks'], first['pair_cross_blocks']))
        for name, _, _ in configs:
            rs = [r[kind] for r in runs[name]]
            row = '  %-8s' % name
            for d in ('fwd', 'bwd'):
                v = np.array([r[d + '_ms'] for r in rs])
                row += '  %s %8.3f (spread %.3f)' % (d, np.median(v), v.max() - v.min())
            tot = np.array([r['fwd_ms'] + r['bwd_ms'] for r in rs])
            row += '  fwd+bwd %8.3f (spread %.3f)  MFMAs fwd %d bwd %d' % (np.median(tot), tot.max() - tot.min(), rs[0]['mfma_fwd'], rs[0]['mfma_bwd'])
            lines.append(row)
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
