"""
Child process of tests/test_alm_gpu.py: the alm2pix adjoint under the environment it was started with.  RIME_ALM_BWD_WIDE and
RIME_ALM_BWD_DMA are read once per process, so the 4-wave packed kernel at MT = 4 and the register-staged kernel at even
pixel counts can only be reached in a process of their own.  Usage: alm_switch_child.py <out>; writes <out>.json -- per case
and mode the plan in force (rime_alm2pix_plan), the worst error / bound against the reference of tests/alm_common.py and
whether two runs gave equal bits -- and <out>.npz with the gradients.
"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import alm_common as ac                              # noqa: E402


def main(out):
    from bayeslim_amd import ops
    dev = torch.device('cuda', 0)
    ops.ALM_SPLIT_F16 = True
    ops.ALM_PACKED_MIN_BYTES = 0
    rec, grads = {}, {}
    for R, Nc, Npix in ac.SWITCH_CASES:
        d = ac.case_data(R, Nc, Npix, 'f32')
        for mode in ('split', 'packed'):
            ops.ALM_PACKED = mode == 'packed'
            Y = torch.as_tensor(np.array(d['Y'])).to(dev)
            res = []
            for _ in range(2):
                x = torch.as_tensor(np.array(d['alm'])).to(dev).requires_grad_(True)
                y = ops.alm2pix(x, Y)
                g, = torch.autograd.grad(y, x, torch.as_tensor(np.array(d['gout'])).to(dev))
                res.append(g.cpu().numpy())
            if mode == 'packed':
                st = ops.ylm_packed_state(Y)
                assert st is not None and st[3].get(1) not in (None, False), 'the packed copy was not used'
            plan = (ctypes.c_int * 6)()
            assert ops.lib.rime_alm2pix_plan(0, d['ys'], R, Nc, Npix, 1, int(mode == 'packed'), plan) == 0
            key = '%s|%s' % (ac.case_id((R, Nc, Npix)), mode)
            rec[key] = dict(plan=list(plan), equal_bits=res[0].tobytes() == res[1].tobytes(),
                            worst=ac.check_backward(res[0], d, Npix, 'f32', True, key))
            grads[key] = res[0]
    np.savez(out + '.npz', **grads)
    with open(out + '.json', 'w') as f:
        json.dump(rec, f)


if __name__ == '__main__':
    main(sys.argv[1])
