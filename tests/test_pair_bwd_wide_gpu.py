"""
The widened pixel splits of the conjugate-pair backward (pair_bwd_split_plan, csrc/fringe_mfma_common.h) against the generic
plan on a real launch: the same cases in two fresh child processes (tests/pair_bwd_wide_child.py), RIME_PAIR_BWD_WIDE=1 and
=0 -- the library reads the switch once.  Each child runs every case three times (bit-identical) and holds sampled (t, f)
rows to the 1e-4 bound of the float64 kernels; here the gradients of the two plans must be the same bytes, the shape must
really widen (rime_fringe_pair_bwd_splits), and the cases must reach the hub / two-tile and the one-tile instantiations with
accumulate 0 and 1.
"""
import json
import os
import subprocess
import sys

import pytest

from pair_bwd_wide_child import CASES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def records(tmp_path_factory):
    d = tmp_path_factory.mktemp('pair_bwd_wide')
    out = {}
    for wide in ('1', '0'):
        path = str(d / ('wide%s.json' % wide))
        env = dict(os.environ, RIME_PAIR_BWD_WIDE=wide)
        r = subprocess.run([sys.executable, os.path.join(HERE, 'pair_bwd_wide_child.py'), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, 'RIME_PAIR_BWD_WIDE=%s:\n%s\n%s' % (wide, r.stdout[-2000:], r.stderr[-4000:])
        with open(path) as f:
            out[wide] = json.load(f)
    return out


@pytest.mark.parametrize('cid,kind', CASES)
def test_wide_and_generic_plan_give_the_same_bits(records, cid, kind):
    w, g = records['1']['%s|%s' % (cid, kind)], records['0']['%s|%s' % (cid, kind)]
    print('%s %s: splits %d (generic %d)  gradient vs float64 %.2e / %.2e  max |g| %.3e' % (
        cid, kind, w['splits'], g['splits'], w['ratio'], g['ratio'], w['gmax']))
    # the shape widens, and each child launched the plan it was asked for
    assert w['generic'] == 5 and w['wide'] == 2
    assert w['splits'] == 2 and g['splits'] == 5
    assert w['gmax'] > 0 and w['nbytes'] == g['nbytes']
    assert w['digest'] == g['digest'], 'the gradient depends on the pixel split'
    assert w['launched'] == g['launched']


def test_cases_reach_both_tile_shapes_and_accumulate(records):
    rows = {r for rec in records['1'].values() for r in rec['launched']}
    assert any(r.startswith('fringe_pair_bwd_kernel<true, true, 2>') for r in rows), rows       # hub, FLAT
    assert any(r.startswith('fringe_pair_bwd_kernel<true, false, 2>') for r in rows), rows      # hub, tilted
    assert any(', 1> ' in r for r in rows), rows                                                # one row tile
    assert any(r.endswith('accumulate=0') for r in rows) and any(r.endswith('accumulate=1') for r in rows), rows
