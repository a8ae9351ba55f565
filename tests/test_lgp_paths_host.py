"""Host-side pieces of lgp.sample_paths (no GPU): its signature, and the refusals of malformed input that it shares with
lgp.predict (raised before any device work)."""
import inspect

import numpy as np
import pytest


def _system():
    """A two-layer system built by hand, as the linked tests do: only the wiring is read before the refusals."""
    from dgp_amd.linkgp import container, lgp
    cs = []
    for idx in (np.array([0, 1]), np.array([0])):
        c = container.__new__(container)
        c.type, c.vecch, c.local_input_idx, c.structure = 'gp', False, idx, None
        cs.append(c)
    sysm = lgp.__new__(lgp)
    sysm.L, sysm.all_layer, sysm.num_model, sysm.all_layer_set = 2, [[cs[0]], [cs[1]]], [1], [[[cs[0]], [cs[1]]]]
    return sysm


def test_lgp_sample_paths_signature():
    from dgp_amd.linkgp import lgp
    p = inspect.signature(lgp.sample_paths).parameters
    assert list(p) == ['self', 'x', 'sample_size', 'full_layer']
    assert p['sample_size'].default == 50 and p['full_layer'].default is False


@pytest.mark.parametrize('method', ['predict', 'sample_paths'])
def test_malformed_input_raises_like_predict(method):
    sysm = _system()
    f = getattr(sysm, method)
    with pytest.raises(Exception, match='numpy 2d-array'):
        f(np.zeros(5))
    with pytest.raises(Exception, match='global inputs to the all layers'):
        f([np.zeros((5, 2))])
    sysm.all_layer[0][0].local_input_idx = [np.array([0])]
    with pytest.raises(Exception, match='first layer, local_input_idx must be a 1d-array'):
        f(np.zeros((5, 2)))
    sysm.all_layer[0][0].local_input_idx = np.array([0, 1])
    if method == 'sample_paths':   # (predict meets a deeper emulator's wiring only after emulating the layers before it)
        sysm.all_layer[1][0].local_input_idx = [np.array([0]), None]
        with pytest.raises(Exception, match='length of 1'):
            f([np.zeros((5, 2)), [None]])
