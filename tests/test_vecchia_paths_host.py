"""Host-side pieces of the Vecchia joint sample paths (no GPU): the public signatures of emulator.sample_paths_vecchia /
gp.sample_paths_vecchia and the C-ABI names of their kernels."""
import ctypes
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('dgpamd_vpaths_nn', 'dgpamd_vpaths_rows')


def test_sample_paths_vecchia_signatures():
    from dgp_amd import emulator, gp
    p = inspect.signature(emulator.sample_paths_vecchia).parameters
    assert list(p) == ['self', 'x', 'sample_size', 'full_layer', 'm']
    assert p['sample_size'].default == 50 and p['full_layer'].default is False and p['m'].default == 50
    p = inspect.signature(gp.sample_paths_vecchia).parameters
    assert list(p) == ['self', 'x', 'sample_size', 'm']
    assert p['sample_size'].default == 50 and p['m'].default == 50


def test_vpaths_entry_points_are_declared_and_exported():
    from dgp_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'dgp_amd.h')).read()
    lib = ctypes.CDLL(os.path.join(ROOT, 'dgp_amd', 'libdgp_amd.so'))
    for name in NAMES:
        assert 'int %s(' % name in src
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
