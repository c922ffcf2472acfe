"""
The merged fringe launch over the sky components of a RIME call (csrc/fringe_mfma.hip, SEGMENTS; ops.fringe_sum_components)
against the per-component launches: the same cases in two fresh child processes (tests/fringe_segments_child.py),
RIME_FRINGE_MERGE=1 and =0 -- the package reads the switch at import.  Each child runs every case three times
(bit-identical) and holds visibilities and gradients to the bounds of the float64 vector-ALU kernels (1e-5 / 1e-4, max-norm
per (t, f) row).  Here: the two paths give the same bytes wherever every segment after the first has one pixel split -- the
slabs are then summed in the order of the per-component reductions and the complex add -- and agree within 2 ulp of the
max-norm otherwise; gradients are the same bytes for every split (pixel tiles are independent outputs).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fringe_segments_child import CASES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LATER_SPLITS = {'later-splits'}                      # cases whose second segment takes more than one forward split


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    out = {}
    for merge in ('1', '0'):
        d = str(tmp_path_factory.mktemp('fringe_segments_%s' % merge))
        r = subprocess.run([sys.executable, os.path.join(HERE, 'fringe_segments_child.py'), d],
                           env=dict(os.environ, RIME_FRINGE_MERGE=merge), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, 'RIME_FRINGE_MERGE=%s:\n%s\n%s' % (merge, r.stdout[-2000:], r.stderr[-4000:])
        print(r.stdout)
        with open(os.path.join(d, 'records.json')) as f:
            out[merge] = (d, json.load(f))
    return out


def test_children_took_the_path_asked_for(runs):
    on, off = runs['1'][1], runs['0'][1]
    assert on['merge'] is True and off['merge'] is False
    for name, (_, pixels, _, needs) in CASES.items():
        e1, e0 = on[name]['entries'], off[name]['entries']
        assert 'rime_fringe_pair_fwd_segments' in e1 and 'rime_fringe_pair_segments_finish' in e1, (name, e1)
        assert not any(e.endswith('_block') or e.endswith('fwd_finish') for e in e1), (name, e1)
        assert 'rime_fringe_pair_fwd_block' in e0 and not any('segments' in e for e in e0), (name, e0)
        # merged, per run: one row scale per component, one forward launch, one reduction; one transpose, one row scale and
        # one backward launch for all components that need a gradient
        assert on[name]['calls'] == len(pixels) + 2 + 3, (name, on[name])
        assert off[name]['calls'] == 3 * len(pixels) + 3 * sum(needs), (name, off[name])


@pytest.mark.parametrize('name', list(CASES))
def test_merged_launch_against_component_launches(runs, name):
    (d1, on), (d0, off) = runs['1'], runs['0']
    a, b = np.load(os.path.join(d1, name + '.npz')), np.load(os.path.join(d0, name + '.npz'))
    print('%s: vis vs float64 %.2e / %.2e, gradients %.2e / %.2e' % (name, on[name]['vis'], off[name]['vis'],
                                                                      on[name]['grad'], off[name]['grad']))
    needs = CASES[name][3]
    assert sorted(a.files) == sorted(b.files) == sorted(['vis'] + ['grad%d' % k for k, n in enumerate(needs) if n])
    for k in a.files:
        if k == 'vis' and name in LATER_SPLITS:
            ulp = np.spacing(np.float32(np.abs(b[k]).max()))
            diff = np.abs(a[k].astype(np.float64) - b[k]).max()
            print('%s: max |merged - per component| %.3e, ulp of the max-norm %.3e' % (name, diff, ulp))
            assert diff <= 2 * ulp
        else:
            assert a[k].tobytes() == b[k].tobytes(), '%s: %s differs between the merged and the per-component path' % (name, k)
        assert np.abs(a[k]).max() > 0


def test_one_segment_is_the_single_plane_entry_point(runs):
    for merge in ('1', '0'):
        rec = runs[merge][1]
        assert rec['two-mixed-pos']['single'] is True and rec['one-tile']['single'] is True
