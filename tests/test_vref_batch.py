"""The batched variational refinement where there is no device: the scratch size from the layout, RefineOptions' defaults, and the
checks of grid_sequence(refine=...) that must arrive before a Context is created."""
import ctypes as C
import os

import numpy as np
import pytest

import vref_batch_probes as P
from wass_amd import _lib, gridding, refinement


def test_scratch_bytes_are_the_layouts():
    lib = _lib.load()
    n = C.c_size_t(0)
    for dims in ((1024, 1024, 2058, 2456, 2058, 2456), (65, 67, 5, 7, 64, 48), (2, 2, 2, 2, 2, 2), (13, 9, 200, 150, 5, 7)):
        want1, shared, frame = P.scratch_bytes(1, *dims)
        assert lib.wass_vref_batch_scratch_bytes(1, *dims, C.byref(n)) == 0 and n.value == want1 == shared + frame, dims
        single = C.c_size_t(0)
        assert lib.wass_vref_scratch_bytes(*dims, C.byref(single)) == 0 and single.value == want1      # a batch of one
        prev = want1
        for nb in (2, 3, 8, 16):
            assert lib.wass_vref_batch_scratch_bytes(nb, *dims, C.byref(n)) == 0
            assert n.value == shared + nb * frame and (n.value - want1) % (nb - 1) == 0 and (n.value - want1) // (nb - 1) == frame
            assert n.value > prev
            prev = n.value
    # the production size: a frame is six planes, two pictures, three coarse planes and the partials
    _, shared, frame = P.scratch_bytes(1, 1024, 1024, 2058, 2456, 2058, 2456)
    # (a picture's 20 217 792 bytes round up to 20 217 856; the tables are 2048 * 12 + 1024 * 20 = 45 056 bytes)
    assert frame == 6 * 4 * 1024 * 1024 + 2 * 20217856 + 3 * 4 * 512 * 512 + 16 * 64 * 16 and shared == 2 * 4 * 1024 * 1024 + 256 + 45056
    for bad in ((0, 8, 8, 8, 8, 8, 8), (-1, 8, 8, 8, 8, 8, 8), (2, 1, 8, 8, 8, 8, 8), (2, 8, 1, 8, 8, 8, 8), (2, 8, 8, 1, 8, 8, 8), (2, 8, 8, 8, 1, 8, 8),
                (2, 8, 8, 8, 8, 1, 8), (2, 8, 8, 8, 8, 8, 1), (2, 40000, 8, 8, 8, 8, 8), (2, 8, 8, 8, 40000, 8, 8), (1, 0, 0, 0, 0, 0, 0)):
        assert lib.wass_vref_batch_scratch_bytes(*bad, C.byref(n)) == -1, bad
    assert lib.wass_vref_batch_scratch_bytes(2, 8, 8, 8, 8, 8, 8, None) == -1


def test_batch_entries_refuse_null_handles_without_a_device():
    lib = _lib.load()
    st, rows = C.c_int64(0), C.c_int(0)
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    zeros = (C.c_double * 12)()
    assert lib.wass_vref_batch_create(None, 2, 8, 8, None, None, C.cast(zeros, dp), C.cast(zeros, dp), C.cast(zeros, dp), C.cast(zeros, dp), 8, 8, 8, 8,
                                      None, C.byref(h)) == -1 and not h.value
    assert lib.wass_vref_batch_load(None, 1, None, None, None, None, 1.0) == -1
    assert lib.wass_vref_batch_set_state(None, None, None, None, 0) == -1 and lib.wass_vref_batch_get_state(None, None, None, None, C.byref(st)) == -1
    assert lib.wass_vref_batch_optimize(None, 1, 10.0, 1e-3, 1e-7, 10, None, 0, C.byref(rows)) == -1
    assert lib.wass_vref_batch_result(None, None, None) == -1
    lib.wass_vref_batch_destroy(None)


def test_refine_options_defaults():
    o = refinement.RefineOptions()
    assert (o.max_iters, o.alpha, o.lr, o.report_every) == (400, 10.0, 1e-3, 10)          # the reference's optimize(): 400, 10, 1e-3
    assert isinstance(o.batch, int) and o.batch >= 1
    assert refinement.RefineOptions(max_iters=7, batch=2).batch == 2
    assert gridding.GridSequenceResult.__dataclass_fields__["refine_losses"].default is None


def _png(path, h, w):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.full((h, w), 90, np.uint8)).save(path)


def _setup(h=12, w=16):
    return {"Rpl": np.eye(3), "Tpl": np.zeros((3, 1)), "CAM_BASELINE": 2.5, "xmin": -1.0, "xmax": 1.0, "ymin": -1.0, "ymax": 1.0,
            "XX": np.zeros((h, w)), "YY": np.zeros((h, w)), "P0cam": np.eye(3, 4), "P1cam": np.eye(3, 4)}


def test_grid_sequence_checks_its_refinement_inputs_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a Context was created before the inputs were checked")
    monkeypatch.setattr(gridding, "Context", no_context)
    dirs = [str(tmp_path / ("%06d_wd" % i)) for i in range(3)]
    for d in dirs:
        for name in ("00000000.png", "00000001.png"):
            _png(os.path.join(d, "undistorted", name), 10, 14)
    opts = refinement.RefineOptions(max_iters=1)
    # missing keys, all named
    setup = _setup()
    del setup["P1cam"], setup["YY"]
    with pytest.raises(ValueError) as e:
        gridding.grid_sequence(dirs, setup, ctx=None, refine=opts)
    assert "P1cam" in str(e.value) and "YY" in str(e.value) and "P0cam" not in str(e.value)
    # a missing picture, named
    gone = os.path.join(dirs[1], "undistorted", "00000001.png")
    os.remove(gone)
    with pytest.raises(FileNotFoundError) as e:
        gridding.grid_sequence(dirs, _setup(), refine=opts)
    assert gone in str(e.value)
    # pictures of two sizes: the frame is named
    _png(gone, 10, 15)
    with pytest.raises(ValueError) as e:
        gridding.grid_sequence(dirs, _setup(), refine=opts)
    assert dirs[1] in str(e.value) and "10 x 15" in str(e.value)
    # all in order: only now a Context is asked for; and without refine nothing of this is read
    _png(gone, 10, 14)
    with pytest.raises(AssertionError, match="Context was created"):
        gridding.grid_sequence(dirs, _setup(), refine=opts)
    os.remove(gone)
    setup = _setup()
    del setup["P0cam"], setup["P1cam"], setup["YY"]
    with pytest.raises(AssertionError, match="Context was created"):
        gridding.grid_sequence(dirs, setup)
