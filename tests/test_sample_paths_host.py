"""Host-side pieces of the joint sample paths (no GPU): the workspace size formula of dgpamd_joint_cov and the public
signatures of emulator.sample_paths / gp.sample_paths."""
import ctypes
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_joint_workspace_holds_both_operands_of_every_item():
    """Per item two (n rounded up to 64) x (M rounded up to 64 + r rounded up to 64) arrays: K(W, x) beside y^T, and
    L^-1 times it."""
    lib = ctypes.CDLL(os.path.join(ROOT, 'dgp_amd', 'libdgp_amd.so'))
    f = lib.dgpamd_joint_workspace
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    up = lambda v: -(-v // 64) * 64
    for n, M, r, batch in ((1, 1, 1, 1), (2000, 1000, 1, 10), (200, 2100, 10, 1), (65, 64, 0, 3), (130, 130, 64, 64)):
        assert f(n, M, r, batch) == 2 * 8 * batch * up(n) * (up(M) + (up(r) if r else 0)), (n, M, r, batch)
    assert f(0, 10, 1, 1) == 0 and f(10, 10, -1, 1) == 0


def test_sample_paths_signatures():
    from dgp_amd import emulator, gp
    p = inspect.signature(emulator.sample_paths).parameters
    assert list(p) == ['self', 'x', 'sample_size', 'full_layer']
    assert p['sample_size'].default == 50 and p['full_layer'].default is False
    p = inspect.signature(gp.sample_paths).parameters
    assert list(p) == ['self', 'x', 'sample_size'] and p['sample_size'].default == 50
