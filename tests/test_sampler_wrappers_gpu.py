"""
GPU checks of the call layer of the five flat-vector wrappers (sampler.hmc_step, nuts.leaf_open, nuts.leaf_close, massmat.project,
massmat.drift): every operand the Python checks refuse, with the exact words of the refusal and before any launch (no tensor is
touched), and that the workspace a wrapper is given does not reach the result: none, one that is too short and a sufficient one
give the same bits.  Vectors of five elements; 4101 float32 elements (one full chunk and a tail of five) for the workspaces.
"""
import pytest
import torch

from bayeslim_amd import _lib, massmat, nuts, sampler

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 5

VECTORS = '%s: contiguous vectors of %s [%d] on %s are needed'
FIRST = '%s: %s takes contiguous real vectors (complex parameters as their interleaved views)'
OUT = '%s: out must be a contiguous float64 tensor of three elements on %s'

# wrapper: (function, the words' module prefix, the vector that sets dtype / length / device, every vector, the other arguments)
WRAPPERS = {
    'hmc_step': (sampler.hmc_step, 'sampler', 'p', ('q', 'p', 'g', 'eps', 'c'), dict(kick=0.5, drift=1.0)),
    'leaf_open': (nuts.leaf_open, 'nuts', 'p0', ('q0', 'p0', 'g0', 'q1', 'p1', 'eps', 'c'), dict(h=0.5)),
    'leaf_close': (nuts.leaf_close, 'nuts', 'p1', ('q1', 'p1', 'g1', 'eps', 'c', 'q_far', 'p_far'), dict(h=0.5)),
    'project': (massmat.project, 'massmat', 'p_in', ('p_in', 'g', 'eps', 'c', 'p_out', 'z'), dict(table=None, kick=0.5)),
    'drift': (massmat.drift, 'massmat', 'z', ('z', 'q_in', 'eps', 'c', 'q_out', 'p', 'q_far', 'p_far'), dict(table=None, drift=1.0)),
}
TAKES_OUT = ('leaf_close', 'drift')


def good(name, dtype=torch.float32, n=N):
    """the arguments of an acceptable call: distinct vectors of n elements, and the three doubles where the wrapper takes them"""
    gen = torch.Generator(device=DEV).manual_seed(11)
    _, _, _, vectors, rest = WRAPPERS[name]
    args = {v: torch.randn(n, generator=gen, device=DEV, dtype=torch.float64).to(dtype) for v in vectors}
    args.update(rest)
    if name in TAKES_OUT:
        args['out'] = torch.full((3,), -7.25, dtype=torch.float64, device=DEV)
    return args


def refused(name, args, words):
    """the call raises ValueError with exactly these words and leaves every tensor as it was"""
    kept = {k: v.clone() for k, v in args.items() if isinstance(v, torch.Tensor)}
    with pytest.raises(ValueError) as e:
        WRAPPERS[name][0](**args)
    assert str(e.value) == words
    assert all(torch.equal(args[k].cpu(), v.cpu()) for k, v in kept.items())


@pytest.mark.parametrize('name', list(WRAPPERS))
def test_a_bad_operand_is_refused_in_the_wrappers_words(name):
    _, prefix, first, vectors, _ = WRAPPERS[name]
    base = good(name)
    words = VECTORS % (prefix, torch.float32, N, base[first].device)
    bad = {'dtype': lambda t: t.double(), 'length': lambda t: torch.cat([t, t[:1]]), 'device': lambda t: t.cpu(),
           'contiguous': lambda t: torch.stack([t, t], 1)[:, 0]}
    for v in vectors:
        if v == first:
            continue
        for what, spoil in bad.items():
            args = dict(base)
            args[v] = spoil(base[v])
            assert what != 'contiguous' or (args[v].numel() == N and not args[v].is_contiguous())
            refused(name, args, words)


@pytest.mark.parametrize('name', list(WRAPPERS))
def test_a_complex_or_strided_first_vector_is_refused(name):
    _, prefix, first, vectors, _ = WRAPPERS[name]
    words = FIRST % (prefix, name)
    args = good(name)
    args.update({v: torch.complex(args[v], args[v]) for v in vectors})          # all complex64: the operands agree, the first is judged
    refused(name, args, words)
    args = good(name)
    args[first] = torch.stack([args[first], args[first]], 1)[:, 0]
    assert args[first].numel() == N and not args[first].is_contiguous()
    refused(name, args, words)


def test_hmc_step_names_an_unsupported_dtype_before_it_judges_the_operands():
    """an int32 p with operands that do not match it: the dtype is refused (TypeError), not the operands (ValueError)"""
    args = good('hmc_step')
    args['p'] = torch.arange(N, dtype=torch.int32, device=DEV)
    kept = {k: v.clone() for k, v in args.items() if isinstance(v, torch.Tensor)}
    with pytest.raises(TypeError) as e:
        sampler.hmc_step(**args)
    assert str(e.value) == 'sampler: float32 / float64 (or complex64 / complex128) parameters only, got %s' % torch.int32
    assert all(torch.equal(args[k], v) for k, v in kept.items())


@pytest.mark.parametrize('name', TAKES_OUT)
def test_a_bad_out_is_refused(name):
    _, prefix, first, _, _ = WRAPPERS[name]
    base = good(name)
    words = OUT % (prefix, base[first].device)
    for out in (torch.zeros(3, dtype=torch.float32, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV),
                torch.zeros(6, dtype=torch.float64, device=DEV)[::2]):
        refused(name, dict(base, out=out), words)


@pytest.mark.parametrize('n,dtype', [(5, torch.float32), (5, torch.float64), (4101, torch.float32)], ids=['5-f32', '5-f64', '4101-f32'])
@pytest.mark.parametrize('name', ['hmc_step', 'leaf_close', 'drift'])
def test_the_workspace_does_not_reach_the_result(name, n, dtype):
    """ws=None and a workspace one double short are replaced inside the wrapper: the sums carry the bits of a sufficient one"""
    need = {'hmc_step': _lib.lib.rime_hmc_workspace, 'leaf_close': _lib.lib.rime_nuts_workspace, 'drift': _lib.lib.rime_mass_workspace}[name](n)
    assert need >= 8 and need % 8 == 0
    key = 'energy' if name == 'hmc_step' else 'out'
    got = []
    for ws in (torch.empty(need // 8, dtype=torch.float64, device=DEV), None, torch.empty(need // 8 - 1, dtype=torch.float64, device=DEV)):
        args = good(name, dtype, n)                                             # fresh: the wrappers write p, q_out
        if name == 'hmc_step':
            args['energy'] = torch.full((1,), -7.25, dtype=torch.float64, device=DEV)
        WRAPPERS[name][0](ws=ws, **args)
        got.append(args[key].view(torch.int64).tolist())
        assert torch.isfinite(args[key]).all() and (args[key] != -7.25).all()
    assert got[0] == got[1] == got[2], got
