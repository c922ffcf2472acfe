#!/usr/bin/env python3
"""
The host cost of one call of each flat-vector wrapper (sampler.hmc_step, nuts.leaf_open / leaf_close, massmat.project / drift):
the Python checks, the ctypes call and the launch, at five elements so that the kernels cost nothing.  5000 calls between two
readings of the host clock, nine times; minimum and median in microseconds per call.  This is the figure a change of the call
layer in sampler.py moves; the trajectory benchmarks (bench_hmc.py, bench_nuts_leaf.py, bench_massmat.py) add the state of the
device and of the process to it.

  python tools/bench_sampler_calls.py [ROOT]      ROOT: another checkout with a built library to measure (default: this one)
"""
import os
import sys
import time

root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402
from bayeslim_amd import sampler, nuts, massmat  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('bench_sampler_calls.py measures on the GPU; none found')
assert os.path.abspath(sampler.__file__).startswith(os.path.abspath(root))
N, dev = 5, 'cuda'
v = lambda: torch.randn(N, device=dev)
q, p, g, q1, p1, qf, pf, z = (v() for _ in range(8))
e = torch.zeros(1, dtype=torch.float64, device=dev); out = torch.zeros(3, dtype=torch.float64, device=dev)
ws = torch.empty(3, dtype=torch.float64, device=dev)
calls = {
 'hmc_step': lambda: sampler.hmc_step(q, p, g, None, None, 1e-3, 1e-3),
 'hmc_step+energy': lambda: sampler.hmc_step(None, p, g, None, None, 1e-3, 0.0, e, ws),
 'leaf_open': lambda: nuts.leaf_open(q, p, g, q1, p1, None, None, 1e-3),
 'leaf_close': lambda: nuts.leaf_close(q1, p1, g, None, None, 1e-3, qf, pf, out, ws),
 'project': lambda: massmat.project(None, p, g, None, None, 1e-3, p1, z),
 'drift+out': lambda: massmat.drift(None, z, q, None, None, 1e-3, q1, p=p1, q_far=qf, p_far=pf, out=out, ws=ws),
}
K = 5000
for name, fn in calls.items():
    for _ in range(500): fn()
    ts = []
    for _ in range(9):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(K): fn()
        t1 = time.perf_counter(); torch.cuda.synchronize()
        ts.append((t1 - t0) / K * 1e6)
    ts.sort()
    print('%-16s host us/call  min %.3f  median %.3f' % (name, ts[0], ts[4]))
