"""Host checks of the bootstrap batch (BootStrap.BSCG(batch=B), csrc/bscg.hip.h): the argument checks and the wavelet
refusal fire before any device work, and the two entry points are in the header, the prototypes and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


class _NoDevice(object):
    """Stands where the engine would: any use of the device fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device work before the argument checks: engine.%s" % name)


def _bootstrap(wavelet=False):
    """A BootStrap with the attributes BSCG reads and no engine behind it (the constructor assembles the kernel)."""
    from gravinv3dhmc_amd.inversion.reginv import BootStrap, _diag
    bs = object.__new__(BootStrap)
    bs.samples, bs.maxk, bs.beta, bs.boundary, bs.wavelet = 3, 5, 0.1, (0.0, 1.0), wavelet
    bs.dsize, bs.msize = 4, 6
    bs.dobs = np.zeros(4)
    bs.Wm = bs.WmInv = bs.WmSquare = _diag(np.ones(6))
    bs._engine = _NoDevice()
    bs._index = None
    return bs


@pytest.mark.parametrize("batch", [0, 17, 2.5, -1, "4", True])
def test_batch_must_be_an_int_in_1_to_16(batch, capsys):
    bs = _bootstrap()
    with pytest.raises(ValueError, match="1..16"):
        bs.BSCG(np.zeros(6), batch=batch)
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("wavelet", ["1D", "3D"])
def test_wavelet_with_batch_is_refused_before_device_work(wavelet, capsys):
    bs = _bootstrap(wavelet)
    with pytest.raises(NotImplementedError, match="bootstrap batch"):
        bs.BSCG(np.zeros(6), batch=4)
    with pytest.raises(NotImplementedError, match="bootstrap batch"):
        bs.CG_batch(np.ones((2, 4)), bs.dobs, np.zeros(6))
    # the argument check comes first
    with pytest.raises(ValueError, match="1..16"):
        bs.BSCG(np.zeros(6), batch=0)
    assert capsys.readouterr().out == ""


def test_batch_reaches_the_device_only_after_the_checks():
    """The stand-in engine is what a valid call trips over: the checks above really ran in front of it."""
    bs = _bootstrap()
    with pytest.raises(AssertionError, match="engine.bscg_run"):
        bs.BSCG(np.zeros(6), batch=2)


def test_default_path_has_no_new_argument_in_its_way():
    import inspect
    from gravinv3dhmc_amd.inversion.reginv import BootStrap
    sig = inspect.signature(BootStrap.BSCG)
    assert list(sig.parameters) == ["self", "initialModel", "batch"] and sig.parameters["batch"].default is None
    assert list(inspect.signature(BootStrap.CG_batch).parameters) == ["self", "counts", "dobs", "initialModel"]


def test_bscg_entry_points_declared_and_exported(built_lib):
    from gravinv3dhmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gravhmc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in ("gh_bscg_run", "gh_bscg_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert len(_lib.PROTOTYPES["gh_bscg_run"][1]) == 16 and len(_lib.PROTOTYPES["gh_bscg_stats"][1]) == 4
