"""Arrays handed to an operator as views into guarded parents, and the check that only the views' cells changed: what
tests/test_cube_staging_gpu.py and tests/test_handle_staging_gpu.py share.  A view is dense in no axis but the last: every second
frame and an inner window of rows and columns of an array whose other cells hold a guard value (a contiguous window of a guarded
vector where an operator wants its output contiguous)."""
import numpy as np

GUARD = {"f": 7.0e30, "u": 0xA5, "i": -77}       # by dtype kind; none of them is a value an operator writes in these tests


def host(v):
    return v.cpu().numpy() if hasattr(v, "data_ptr") else np.asarray(v)


def _window(parent, shape, dense):
    """the view of `shape` inside a parent made by _parent; numpy and torch slice alike"""
    return parent[32:-32].reshape(shape) if dense else parent[::2, ..., 2:-1, 3:-2]


def _parent(shape, dtype, dense, dev):
    """(parent, view, inside): an array of guard cells, on the device if `dev`, its view of `shape` and which cells the view covers"""
    dtype = np.dtype(dtype)
    full = (int(np.prod(shape)) + 64,) if dense else (2 * shape[0],) + tuple(shape[1:-2]) + (shape[-2] + 3, shape[-1] + 5)
    parent = np.full(full, GUARD[dtype.kind], dtype)
    inside = np.zeros(full, bool)
    _window(inside, shape, dense)[...] = True
    if dev:
        import torch
        parent = torch.from_numpy(parent).cuda()
    return parent, _window(parent, shape, dense), inside


class Guarded:
    """arrays handed to an operator as views into guarded parents, and the check that only the views' cells changed"""

    def __init__(self, dev):
        self.dev, self.kept = dev, []

    def input(self, a):
        parent, view, _ = _parent(a.shape, a.dtype, False, self.dev)
        if self.dev:
            import torch
            view.copy_(torch.from_numpy(np.array(a)))              # a copy: the cached inputs are read-only
        else:
            view[...] = a
        self.kept.append((parent, host(parent).copy(), None))       # an input: no cell at all may change
        return view

    def out(self, shape, dtype, dense=False):
        parent, view, inside = _parent(shape, dtype, dense, self.dev)
        self.kept.append((parent, host(parent).copy(), inside))
        return view

    def check(self, what):
        for parent, before, inside in self.kept:
            now = host(parent)
            same = now == before if inside is None else (now == before) | inside
            assert same.all(), f"{what}: {int((~same).sum())} guard cells of {'an input' if inside is None else 'an output'}'s parent changed"
