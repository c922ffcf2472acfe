"""
ParamDict: a dictionary of named parameter tensors with element-wise arithmetic, the container the sampler (sampler.py) moves
positions, momenta, gradients and step sizes in.  Same interface as the reference's paramdict.py; host-side only, no kernel:
every operation is the torch operation applied key by key.

An operand of a binary operation may be a scalar, a tensor (applied to every key) or another ParamDict (matched by key, over
the keys of the left operand).
"""
import operator as _op
import os
import pickle

import torch

from . import utils


class ParamDict:
    """
    params : dict of str -> tensor.  The dict is held, not copied; `devices` records where every tensor lives.
    """
    def __init__(self, params):
        self.params = params
        self._setup()

    def _setup(self):
        self.devices = {k: self.params[k].device for k in self.keys()}

    # ------------------------------------------------------------------ the dictionary
    def keys(self):
        return list(self.params.keys())

    def values(self):
        return list(self.params.values())

    def items(self):
        return list(self.params.items())

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.params)

    def __contains__(self, key):
        return key in self.params

    def __getitem__(self, key):
        return self.params[key]

    def __setitem__(self, key, val):
        self.params[key] = val

    def __repr__(self):
        return 'ParamDict(%s)' % ', '.join('%s: %s%s' % (k, v.dtype, list(v.shape)) for k, v in self.items())

    def update(self, other):
        for key in other:
            self[key] = other[key]
        self._setup()

    # ------------------------------------------------------------------ copies
    def clone(self, **kwargs):
        """clone every tensor (stays in the autograd graph)"""
        return ParamDict({k: v.clone(**kwargs) for k, v in self.items()})

    def copy(self):
        """detach and clone every tensor; a tensor that requires grad comes back as a Parameter"""
        out = {}
        for k, v in self.items():
            c = v.detach().clone()
            out[k] = torch.nn.Parameter(c) if v.requires_grad else c
        return ParamDict(out)

    def detach(self):
        """detach every tensor (shares storage)"""
        return ParamDict({k: v.detach() for k, v in self.items()})

    def ones(self):
        """a clone filled with ones"""
        out = self.clone()
        for k in out:
            out[k][:] = 1.0
        return out

    def push(self, device, inplace=True, copy=True):
        """
        Move every tensor to `device` (a device, a dtype, or a dict of either per key).  inplace: change this object and
        return None; otherwise work on self.copy() (copy=True) or self.clone() and return it.
        """
        obj = self if inplace else (self.copy() if copy else self.clone())
        for k in obj.keys():
            obj.params[k] = utils.push(obj.params[k], device[k] if isinstance(device, dict) else device)
        obj._setup()
        if not inplace:
            return obj

    # ------------------------------------------------------------------ files
    def write_pkl(self, fname, overwrite=False):
        """pickle a clone of this object to fname; an existing file is kept unless overwrite"""
        if os.path.exists(fname) and not overwrite:
            print('{} exists, not overwriting...'.format(fname))
            return
        with open(fname, 'wb') as f:
            pickle.dump(self.clone(), f, protocol=4)

    @staticmethod
    def read_pkl(fname, force_cpu=False):
        """load what write_pkl wrote; force_cpu moves every tensor to the CPU"""
        with open(fname, 'rb') as f:
            pd = pickle.load(f)
        if force_cpu:
            for k in pd.keys():
                pd.params[k] = pd.params[k].cpu()
        pd._setup()
        return pd

    # ------------------------------------------------------------------ functions and arithmetic
    def operator(self, func, args=(), inplace=False):
        """
        func(self[k], *args) for every key; an argument that is a dict or a ParamDict contributes its entry k.  Returns a new
        ParamDict, or with inplace stores the results in this one and returns None.
        """
        out = {}
        for k in self.keys():
            out[k] = func(self[k], *[a[k] if isinstance(a, (dict, ParamDict)) else a for a in args])
        if inplace:
            for k, v in out.items():
                self[k] = v
            return None
        return ParamDict(out)

    def _binary(self, fn, other, reflected=False):
        out = {}
        for k, v in self.items():
            o = other[k] if isinstance(other, ParamDict) else other
            out[k] = fn(o, v) if reflected else fn(v, o)
        return ParamDict(out)

    def _inplace(self, fn, other):
        for k in self.keys():
            self.params[k] = fn(self.params[k], other[k] if isinstance(other, ParamDict) else other)
        return self

    def __add__(self, other):
        return self._binary(_op.add, other)

    def __radd__(self, other):
        return self._binary(_op.add, other, reflected=True)

    def __iadd__(self, other):
        return self._inplace(_op.iadd, other)

    def __sub__(self, other):
        return self._binary(_op.sub, other)

    def __rsub__(self, other):
        return self._binary(_op.sub, other, reflected=True)

    def __isub__(self, other):
        return self._inplace(_op.isub, other)

    def __mul__(self, other):
        return self._binary(_op.mul, other)

    def __rmul__(self, other):
        return self._binary(_op.mul, other, reflected=True)

    def __imul__(self, other):
        return self._inplace(_op.imul, other)

    def __truediv__(self, other):
        return self._binary(_op.truediv, other)

    def __rtruediv__(self, other):
        return self._binary(_op.truediv, other, reflected=True)

    def __itruediv__(self, other):
        return self._inplace(_op.itruediv, other)

    __div__, __rdiv__, __idiv__ = __truediv__, __rtruediv__, __itruediv__

    def __matmul__(self, other):
        return self._binary(_op.matmul, other)

    def __rmatmul__(self, other):
        return self._binary(_op.matmul, other, reflected=True)

    def __imatmul__(self, other):
        return self._inplace(_op.matmul, other)

    def __pow__(self, alpha):
        return self._binary(_op.pow, alpha)

    def __neg__(self):
        return ParamDict({k: -v for k, v in self.items()})


def model2pdict(model, parameters=True, clone=False, prefix=None):
    """
    The `params` tensors of a model and of all its sub-modules as a ParamDict keyed by their dotted names
    ('sky.params', ...).  parameters: only those that require grad; clone: detached clones instead of the model's own tensors;
    prefix: prepended to every key.
    """
    prefix = '' if prefix is None else prefix
    d = {}
    own = getattr(model, 'params', None)
    if own is not None and (not parameters or own.requires_grad):
        d[prefix + 'params'] = own.detach().clone() if clone else own
    for name, child in model.named_children():
        d.update(model2pdict(child, parameters=parameters, clone=clone, prefix='%s%s.' % (prefix, name)).params)
    return ParamDict(d)
