"""Host-side pieces of lgp.sample_paths_vecchia (no GPU): its signature, and the refusals of malformed input that it shares
with lgp.predict and lgp.sample_paths, and of m < 1 (all raised before any device work)."""
import inspect

import numpy as np
import pytest

from test_lgp_paths_host import _system


def test_lgp_sample_paths_vecchia_signature():
    from dgp_amd.linkgp import lgp
    p = inspect.signature(lgp.sample_paths_vecchia).parameters
    assert list(p) == ['self', 'x', 'sample_size', 'full_layer', 'm']
    assert p['sample_size'].default == 50 and p['full_layer'].default is False and p['m'].default == 50


def test_malformed_input_raises_like_predict():
    sysm = _system()
    f = sysm.sample_paths_vecchia
    with pytest.raises(Exception, match='numpy 2d-array'):
        f(np.zeros(5))
    with pytest.raises(Exception, match='global inputs to the all layers'):
        f([np.zeros((5, 2))])
    sysm.all_layer[0][0].local_input_idx = [np.array([0])]
    with pytest.raises(Exception, match='first layer, local_input_idx must be a 1d-array'):
        f(np.zeros((5, 2)))
    sysm.all_layer[0][0].local_input_idx = np.array([0, 1])
    sysm.all_layer[1][0].local_input_idx = [np.array([0]), None]
    with pytest.raises(Exception, match='length of 1'):
        f([np.zeros((5, 2)), [None]])
    sysm.all_layer[1][0].local_input_idx = np.array([0])


@pytest.mark.parametrize('m', [0, -3])
def test_conditioning_set_size_below_one_raises(m):
    sysm = _system()
    with pytest.raises(ValueError, match='at least 1'):
        sysm.sample_paths_vecchia(np.zeros((5, 2)), m=m)
    with pytest.raises(ValueError, match='at least 1'):
        sysm.sample_paths_vecchia([np.zeros((5, 2)), [None]], sample_size=3, full_layer=True, m=m)


def test_dense_refusal_of_a_vecchia_emulator_points_to_the_vecchia_method():
    sysm = _system()
    sysm.all_layer[0][0].vecch = True
    with pytest.raises(NotImplementedError, match='emulator 1 of layer 1') as err:
        sysm.sample_paths(np.zeros((5, 2)))
    assert 'sample_paths_vecchia' in str(err.value) and 'set_vecchia(False)' in str(err.value)
