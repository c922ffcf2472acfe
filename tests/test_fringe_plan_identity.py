"""
The host plan of the matrix-core fringe path, held bit for bit: tests/golden/fringe_plan_digests.json keeps one
sha256 per array of what plan_digest() below hashes.  A digest covers every table (direct, conj, centre, pos, self_pos, the `bwd`
tables of a pair block, both two-pass masks) and every scalar key of every block list of `geom.ant`, the key sets themselves,
what _block_launch makes of each block, and the block builders driven on hand-built blocks, whose tables they read back from the
device.  No GPU: FringeGeometry._setup_antenna_path runs on a stand-in object whose tensors live on the CPU.  The pair cross
plan: hex-169 and hex-217 have two groups, hex-271 three, hex-397 four.
"""
import hashlib
import json
import os
import types

import numpy as np
import pytest
import torch

from bayeslim_amd import ops, utils
from pair_cross_cases import make_array, seed_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fringe_plan_digests.json')
BLOCK_TABLES = ('direct', 'conj', 'centre', 'pos', 'self_pos')
BLOCK_SCALARS = ('nrows', 'cross', 'mp', 'mirror', 'cpass', 'fwd_cpass', 'mf_fwd', 'mf_bwd', 'mf_bwd_real', 'mf_self', 'pair',
                 'xpair', 'flat', 'rows', 'firsts', 'partner', 'hub', 'rows_i', 'rows_j')
ANT_LISTS = ('blocks', 'blocks_mirror', 'blocks_real', 'blocks_cplx')
ANT_SCALARS = ('mirror_groups', 'pair_blocks', 'pair_cross_blocks', 'mfma_fwd', 'mfma_bwd', 'mfma_flops_fwd', 'mfma_flops_bwd',
               'multi_model', 'Nant')


def _hex(side, outrigger=False):
    v = np.asarray(utils._make_hex(side, D=14.6)[1], dtype=np.float64)
    return np.vstack([v, [[250.0, 0.0, 0.0]]]) if outrigger else v


def _pairs(n, rng=None, autos=()):
    """every pair once, in antenna order (rng: each in a random orientation), then the autocorrelations asked for"""
    return [(i, j) if rng is None or rng.random() < 0.5 else (j, i) for i in range(n) for j in range(i + 1, n)] + [(a, a) for a in autos]


def _mirrored(rng, half, single, zscale):
    h = rng.normal(0, 60.0, (half, 3)) * [1, 1, zscale]
    ant = np.vstack([h, -h, rng.normal(0, 60.0, (single, 3)) * [1, 1, zscale]])
    return ant[rng.permutation(len(ant))] + [31.7, -12.3, 4.1]


def _case(kind):
    """(antenna positions, baselines, keywords of _setup_antenna_path) of one array"""
    rng = np.random.default_rng(seed_of(kind, 100))
    kw = {}
    if kind in ('hex19', 'hex37'):                              # one tile, mirror only / pair form, 32 rows, no hub
        ant = _hex(3 if kind == 'hex19' else 4)
        bls = _pairs(len(ant))
    elif kind == 'hera128':                                     # the headline: 64 rows + hub, the backward in its own row order
        ant = _hex(7, True)
        bls = _pairs(128)
    elif kind == 'hera128_mixed':                               # ... all pairs in random orientation
        ant = _hex(7, True)
        bls = _pairs(128, rng)
    elif kind == 'hera128_hub_auto':                            # ... the hub's autocorrelation asked for: no pair form
        ant = _hex(7, True)
        hub = int(np.argmin(np.abs(ant).max(1)))
        bls = _pairs(128, rng, autos=(5, hub))
    elif kind in ('hex169', 'hex217', 'hex271', 'hex397'):      # pair cross plan: two, two, three and four groups
        ant = _hex({'hex169': 8, 'hex217': 9, 'hex271': 10, 'hex397': 12}[kind])
        ant = ant[rng.permutation(len(ant))] + [31.7, -12.3, 4.1]
        bls = _pairs(len(ant), rng)
    elif kind == 'hex169_tilted':                               # ... out of the plane z = const: no `flat` licence
        ant = make_array('hex169t', rng)
        bls = _pairs(len(ant), rng)
    elif kind == 'rand200':                                     # 90 mirror pairs + 20 antennas without a partner
        ant = make_array('rand200', rng)
        bls = _pairs(200, rng)
    elif kind == 'plain140':                                    # no symmetry: plain diagonal and cross blocks
        ant = rng.normal(0, 90.0, (140, 3)) * [1, 1, 0.05]
        bls = [p for p in _pairs(140, rng) if rng.random() < 0.9]
    elif kind == 'two_models128':                               # two beam models on a hexagon: one block per model pair
        ant = _hex(7, True)
        model = [int(a % 3 == 0) for a in range(128)]
        bls = _pairs(128, rng)
        uniq = sorted({(model[a], model[b]) for a, b in bls})
        kw = dict(bl_mp=[uniq.index((model[a], model[b])) for a, b in bls], mp_pairs=uniq)
    elif kind == 'group32':                                     # rank-local tile shards: one-tile blocks
        ant = _hex(7, True)
        bls = _pairs(128)
        kw = dict(group=32)
    elif kind in ('sym100_flat', 'sym100_3d'):                  # 45 pairs + 10 singles, coplanar (flat = 1) or not (flat = 0)
        ant = _mirrored(rng, 45, 10, 0.0 if kind == 'sym100_flat' else 0.3)
        bls = _pairs(100, rng)
    return ant, bls, kw


CASES = ('hex19', 'hex37', 'hera128', 'hera128_mixed', 'hera128_hub_auto', 'hex169', 'hex217', 'hex271', 'hex397', 'hex169_tilted',
         'rand200', 'plain140', 'two_models128', 'group32', 'sym100_flat', 'sym100_3d')


class _Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def put(self, name, x):
        if torch.is_tensor(x):
            x = x.detach().cpu().numpy()
        if isinstance(x, np.ndarray):
            x = np.ascontiguousarray(x)
            body = ('%s%s' % (x.dtype.str, x.shape)).encode() + x.tobytes()
        elif isinstance(x, (list, tuple)):
            body = repr([(int(v) if isinstance(v, (int, np.integer)) else v) for v in x]).encode()
        else:
            body = repr(int(x) if isinstance(x, (bool, np.integer)) else x).encode()
        self.h.update(name.encode() + b'=' + body + b';')

    def block(self, tag, blk):
        self.put(tag + '.keys', sorted(blk))
        for k in BLOCK_TABLES + BLOCK_SCALARS:
            self.put('%s.%s' % (tag, k), blk.get(k, 'absent'))
        bwd = blk.get('bwd')
        self.put(tag + '.bwd', 'absent' if 'bwd' not in blk else bwd is not None)
        if bwd is not None:
            self.put(tag + '.bwd.keys', sorted(bwd))
            for k in ('firsts', 'partner', 'pos', 'direct', 'conj', 'centre'):
                self.put('%s.bwd.%s' % (tag, k), bwd[k])

    def launches(self, tag, blk):
        """what _block_launch makes of a block, as _fringe_ant_call asks: real passes, and the single complex pass where one exists"""
        asks = [(False, 0), (True, 0)] + [(back, blk[k]) for back, k in ((False, 'fwd_cpass'), (True, 'cpass')) if blk[k] != 0]
        for back, cflag in asks:
            name, lead, tables, flag, mf = ops._block_launch(blk, back, cflag)
            self.put('%s.launch%d%+d' % (tag, back, cflag),
                     [name, [x if isinstance(x, int) else bool(x.value) for x in lead], len(tables), list(flag), mf])


def _hand_built(raw, ant):
    """a diagonal block as the tests build one by hand: device tables only (tests/test_host_logic.py, _pair_form_emulated)"""
    blk = dict(nrows=len(raw['ants_i']), cross=0, mp=raw['mp'], cpass=raw['cpass'],
               direct=torch.as_tensor(raw['direct'].reshape(-1)), conj=torch.as_tensor(raw['conj'].reshape(-1)))
    return blk, ant[np.asarray(raw['ants_i'])]


def plan_digest(kind):
    ant, bls, kw = _case(kind)
    d = _Digest()
    # the numpy-in, numpy-out helpers
    plan = ops._pair_cross_plan(ant, bls)
    d.put('cost', list(ops._plain_plan_cost(ant, bls, kw.get('group', ops.MFMA_GROUP))))
    d.put('plan', plan is not None)
    if plan is not None:
        d.put('plan.centre', plan['centre'])
        d.put('plan.ants', [list(map(int, g)) for g in plan['ants']])
        for g, grp in enumerate(plan['groups']):
            d.put('plan.g%d' % g, [list(map(int, grp['firsts'])), list(map(int, grp['partner']))])
        for key in sorted(plan['cross']):
            x = plan['cross'][key]
            d.put('plan.x%s.keys' % (key,), sorted(x))
            for k in ('rows_i', 'rows_j', 'pos', 'flat', 'direct', 'conj'):
                d.put('plan.x%s.%s' % (key, k), x[k])
    raw = ops._antenna_blocks(bls, len(ant), group=kw.get('group', ops.MFMA_GROUP), groups=None if plan is None else plan['ants'])
    for n, r in enumerate(raw):
        d.put('raw%d' % n, [r['ants_i'], r['ants_j'], r['rows_i'], r['rows_j'], r['mp'], r['gi'], r['gj'], r['cpass']])
        d.put('raw%d.direct' % n, r['direct'])
        d.put('raw%d.conj' % n, r['conj'])
        if r['ants_j'] is None:
            # the builders on a block without a host copy of its tables
            blk, P = _hand_built(r, ant)
            order = ops._mirror_order(P)
            d.put('order%d' % n, 'none' if order is None else [list(order[0]), order[1]])
            if order is not None:
                d.put('order%d.c' % n, order[2])
            for ap in (False, True):
                lay = ops._pair_layout(P, ap=ap) if len(P) > 64 else ops._pair_layout(P, rows=32, hub_ok=False, ap=ap)
                d.put('layout%d.%d' % (n, ap), 'none' if lay is None else [list(map(int, lay[0])), list(map(int, lay[1])), lay[2]])
                if lay is not None:
                    d.put('layout%d.%d.c' % (n, ap), lay[3])
                    d.put('ap%d.%d' % (n, ap), list(map(int, ops._pair_ap_order(P[lay[0]] - lay[3]))))
            for name, fn in (('mirror', ops._mirror_block), ('pair', ops._pair_block)):
                out = fn(blk, P, 'cpu')
                d.put('%s%d' % (name, n), out is not None)
                if out is not None:
                    d.block('%s%d' % (name, n), out)
    # the plan as FringeGeometry builds it
    P = torch.as_tensor(ant, dtype=torch.float64)
    i1, i2 = torch.as_tensor([a for a, _ in bls]), torch.as_tensor([b for _, b in bls])
    geom = types.SimpleNamespace(Nbl=len(bls), Nt=2, Nf=3, Pstride=64, blvecs=P[i2] - P[i1], ant=None)
    ops.FringeGeometry._setup_antenna_path(geom, P, bls, force=True, **kw)
    a = geom.ant
    d.put('ant', a is not None)
    if a is not None:
        d.put('ant.keys', sorted(a))
        for k in ANT_SCALARS + ('two_pass_mask', 'two_pass_mask_cplx'):
            d.put('ant.' + k, a.get(k, 'absent'))
        for name in ANT_LISTS:
            d.put('ant.%s.len' % name, len(a[name]) if name in a else 'absent')
            for n, blk in enumerate(a.get(name, ())):
                d.block('%s%d' % (name, n), blk)
                d.launches('%s%d' % (name, n), blk)
    return d.h.hexdigest(), a


@pytest.mark.parametrize('kind', CASES)
def test_plan_is_bit_for_bit_the_recorded_one(kind):
    """every table and scalar of the plan, through FringeGeometry._setup_antenna_path and through the block builders on
    hand-built blocks; and the branch each array is there for is the branch it takes"""
    digest, a = plan_digest(kind)
    assert digest == json.load(open(GOLDEN))[kind]
    kinds = lambda name: [('xpair' if b.get('xpair') else 'pair' if b.get('pair') else 'mirror' if b['mirror'] else 'plain')
                          for b in a.get(name, a['blocks'])]
    real = kinds('blocks_real')
    want = {'hex19': ['mirror'], 'hex37': ['pair'], 'hera128': ['pair'], 'hera128_mixed': ['pair'], 'hera128_hub_auto': ['mirror'],
            'hex169': ['pair', 'xpair', 'pair'], 'hex217': ['pair', 'xpair', 'pair'], 'hex271': ['pair', 'xpair', 'xpair', 'pair', 'xpair', 'pair'],
            'hex397': ['pair', 'xpair', 'xpair', 'xpair', 'pair', 'xpair', 'xpair', 'pair', 'xpair', 'pair'],
            'hex169_tilted': ['pair', 'xpair', 'pair'], 'rand200': ['pair', 'xpair', 'pair'], 'plain140': ['plain'] * 3,
            'group32': ['mirror', 'plain', 'plain', 'plain', 'mirror', 'plain', 'plain', 'mirror', 'plain', 'mirror'],
            'sym100_flat': ['pair'], 'sym100_3d': ['pair']}
    if kind in want:
        assert real == want[kind]
    if kind.startswith('hera128') and kind != 'hera128_hub_auto':
        blk = a['blocks_real'][0]
        assert blk['nrows'] == 64 and blk['hub'] is not None and blk['bwd'] is not None and blk['centre'] is not None
        assert a['blocks_cplx'][0] is blk and 'two_pass_mask_cplx' in a
    if kind == 'hex37':
        assert a['blocks_real'][0]['nrows'] == 19 and a['blocks_real'][0]['hub'] is None
    if kind == 'hera128_hub_auto':
        assert 'blocks_cplx' not in a and a['pair_blocks'] == []
    if kind == 'two_models128':
        assert a['multi_model'] and len({b['mp'] for b in a['blocks']}) == 4
    if kind in ('sym100_flat', 'hex169'):
        assert all(b['flat'] == 1 for b in a['blocks_real'])
    if kind in ('sym100_3d', 'hex169_tilted'):
        assert all(b['flat'] == 0 for b in a['blocks_real'])
    if kind == 'plain140':
        assert sorted(a) == sorted(['blocks', 'Nant', 'mfma_fwd', 'mfma_bwd', 'two_pass_mask', 'mfma_flops_fwd', 'mfma_flops_bwd', 'multi_model'])
    assert a['mfma_fwd'] == sum(b['mf_fwd'] for b in a.get('blocks_real', a['blocks']))
    assert a['mfma_bwd'] == sum(b['mf_bwd_real'] for b in a.get('blocks_real', a['blocks']))


def _tables(n, rng):
    """plain tables of a diagonal block of n antennas, every pair in a random orientation, and its slots"""
    od, oc = (np.full((128, 128), -1, dtype=np.int32) for _ in range(2))
    pairs = [(i, j) for i in range(n) for j in range(i, n)]
    for b, (i, j) in enumerate(pairs):
        (od if (i // 32 < j // 32 or rng.random() < 0.5) else oc)[i, j] = b
    return od, oc, len(pairs)


def test_remapper_alone():
    """ops._remap_tables: every slot of the plain block exactly once in direct / conj / centre under any one-to-one row map, the
    hub's baselines in `centre`, its autocorrelation None; a row map that doubles a row (two slots in one cell, one lost) or
    drops an antenna (no row) raises"""
    rng = np.random.default_rng(0)
    n = 70
    od, oc, nbl = _tables(n, rng)
    vrow = rng.permutation(128)[:n]
    direct, conj, centre = ops._remap_tables(od, oc, vrow)
    assert centre is None and direct.dtype == conj.dtype == np.int32 and direct.shape == conj.shape == (128, 128)
    assert np.array_equal(np.sort(np.concatenate([direct[direct >= 0], conj[conj >= 0]])), np.arange(nbl))
    for i, j in zip(*np.nonzero(od >= 0)):                     # baseline i -> j: direct[r_i, r_j], or conj[r_j, r_i] below the tile diagonal
        r1, r2 = vrow[i], vrow[j]
        assert (direct[r1, r2] if r1 // 32 <= r2 // 32 else conj[r2, r1]) == od[i, j]
    for i, j in zip(*np.nonzero(oc >= 0)):                     # baseline j -> i
        r1, r2 = vrow[j], vrow[i]
        assert (direct[r1, r2] if r1 // 32 <= r2 // 32 else conj[r2, r1]) == oc[i, j]
    hub = 11
    od2, oc2 = od.copy(), oc.copy()
    od2[hub, hub] = oc2[hub, hub] = -1
    hrow = vrow.copy()
    hrow[hub] = -1
    direct, conj, centre = ops._remap_tables(od2, oc2, hrow, hub)
    assert centre.shape == (2, 128) and int((centre >= 0).sum()) == n - 1
    slots = np.concatenate([t[t >= 0] for t in (direct, conj, centre)])
    assert np.array_equal(np.sort(slots), np.sort(np.concatenate([od2[od2 >= 0], oc2[oc2 >= 0]])))
    for a in range(n):
        if a != hub:
            out, back = (od2[hub, a], oc2[hub, a]) if hub < a else (oc2[a, hub], od2[a, hub])     # hub -> a, a -> hub
            assert centre[0, hrow[a]] == out and centre[1, hrow[a]] == back
    assert ops._remap_tables(od, oc, hrow, hub) is None        # the hub's autocorrelation
    doubled = vrow.copy()
    doubled[5] = doubled[9]
    with pytest.raises(AssertionError):
        ops._remap_tables(od, oc, doubled)
    dropped = vrow.copy()
    dropped[5] = -1
    with pytest.raises(AssertionError):
        ops._remap_tables(od, oc, dropped)


def test_mirror_block_applies_the_full_check(monkeypatch):
    """_mirror_block sends its tables through the remapper with its row map (seen by a wrapper around it), so it gets the
    exactly-once check that test_remapper_alone exercises.  A row order that holds one antenna twice and another nowhere raises
    as well, but already at _mirror_block's own every-antenna-has-a-row assert: an antenna-to-row map cannot put two antennas
    into one row, so no row order reaches the remapper's check alone"""
    P = _hex(4)
    od, oc, _ = _tables(len(P), np.random.default_rng(1))
    blk = dict(nrows=len(P), cross=0, mp=0, direct=torch.as_tensor(od.reshape(-1)), conj=torch.as_tensor(oc.reshape(-1)))
    calls, remap = [], ops._remap_tables

    def spy(*args):
        calls.append(args)
        return remap(*args)
    monkeypatch.setattr(ops, '_remap_tables', spy)
    mb = ops._mirror_block(blk, P, 'cpu')
    assert mb is not None and len(calls) == 1
    assert np.array_equal(calls[0][0].reshape(128, 128), od) and np.array_equal(calls[0][1].reshape(128, 128), oc)
    assert [int(r) for r in calls[0][2]] == [mb['rows'].index(a) for a in range(len(P))]
    good = ops._mirror_order

    def bad(P, packed=None):
        rows, mask, c = good(P, packed)
        rows = list(rows)
        rows[rows.index(7)] = 3                                   # antenna 3 in two rows, antenna 7 in none
        return rows, mask, c
    monkeypatch.setattr(ops, '_mirror_order', bad)
    with pytest.raises(AssertionError):
        ops._mirror_block(blk, P, 'cpu')
