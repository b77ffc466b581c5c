"""Small tensor helpers used by the ops (subset of the reference's torch_utils/misc.py)."""

import contextlib
import warnings
import weakref

import torch


def _stamp(t):
    """What has to be unchanged for a tensor derived from parameter `t` to be still valid: `Module.to(device)` and
    `param.data = ...` keep the Parameter object and its `_version` but change the storage, so device and address count."""
    return (t._version, t.device, t.data_ptr())


class DerivedCache:
    """Tensors derived from parameters, kept between calls so that inference does not recompute them and so that a captured
    hipGraph and the packed-weight copies in the HIP workspaces keep pointing at valid memory.  The rules:
    1. an entry is valid only for the very tensor objects it was made from (ids and storage addresses get recycled), at the same `_stamp`;
    2. a live entry is never freed (a captured graph holds raw pointers into it; a blanket `.clear()` would leave its replays reading
       freed memory): only entries whose first source is gone are dropped, and only once the table has outgrown `limit`;
    3. (the caller's) with grad enabled and a source that requires grad nothing is cached: it returns its differentiable expression."""

    def __init__(self, limit=512):
        self.limit, self.table = limit, {}     # key -> (weak references to the sources, (their stamps, extra), value)

    def get(self, sources, build, *, key=None, extra=None):
        """The value `build()` made from the tensors `sources`.  `key` joins id(sources[0]) in the table key (several values per source),
        `extra` is compared together with the stamps (a value that also depends on a number)."""
        k = id(sources[0]) if key is None else (id(sources[0]), key)
        stamp = (*map(_stamp, sources), extra)
        ent = self.table.get(k)
        if ent is not None and ent[1] == stamp:
            for ref, t in zip(ent[0], sources):
                if ref() is not t:
                    break
            else:
                return ent[2]
        if len(self.table) > self.limit:
            for dead in [d for d, e in self.table.items() if e[0][0]() is None]:
                del self.table[dead]
        ent = self.table[k] = (tuple(map(weakref.ref, sources)), stamp, build())
        return ent[2]


@contextlib.contextmanager
def suppress_tracer_warnings():
    """Silence torch.jit.TracerWarning inside the block (reference: misc.py:71)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=torch.jit.TracerWarning)
        yield


def assert_shape(tensor, ref_shape):
    """Check `tensor.shape` against `ref_shape`; `None` entries are wildcards (reference: misc.py:82)."""
    if tensor.ndim != len(ref_shape):
        raise AssertionError(f'Wrong number of dimensions: got {tensor.ndim}, expected {len(ref_shape)}')
    for idx, (size, ref) in enumerate(zip(tensor.shape, ref_shape)):
        if ref is None:
            continue
        if isinstance(ref, torch.Tensor):
            with suppress_tracer_warnings():
                torch._assert(torch.equal(torch.as_tensor(size), ref), f'Wrong size for dimension {idx}')
        elif isinstance(size, torch.Tensor):
            with suppress_tracer_warnings():
                torch._assert(torch.equal(size, torch.as_tensor(ref)), f'Wrong size for dimension {idx}: expected {ref}')
        elif size != ref:
            raise AssertionError(f'Wrong size for dimension {idx}: got {size}, expected {ref}')


def profiled_function(fn):
    """Wrap `fn` in a torch profiler range named after it (reference: misc.py:100)."""
    def decorator(*args, **kwargs):
        with torch.autograd.profiler.record_function(fn.__name__):
            return fn(*args, **kwargs)
    decorator.__name__ = fn.__name__
    decorator.__doc__ = fn.__doc__
    return decorator


def named_params_and_buffers(module):
    assert isinstance(module, torch.nn.Module)
    return list(module.named_parameters()) + list(module.named_buffers())


def copy_params_and_buffers(src_module, dst_module, require_all=False):
    """Copy same-named tensors from src to dst (reference: misc.py:155)."""
    src = dict(named_params_and_buffers(src_module))
    for name, tensor in named_params_and_buffers(dst_module):
        assert (name in src) or (not require_all), f'missing tensor {name}'
        if name in src:
            tensor.copy_(src[name].detach()).requires_grad_(tensor.requires_grad)
