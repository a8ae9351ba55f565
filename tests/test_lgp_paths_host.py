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


def test_connect_cols_places_a_deeper_node_s_global_columns():
    """pathwalk.connect_cols, the input assembly that pathwalk.walk and pathwalk.moments share, against connect_split's cases
    (linkgp.py:538-560): a deterministic input is indexed by `connect` as it stands; a Gaussian one of D = 3 columns with
    external columns behind it splits a middle layer's `connect` at D, and matches the last layer's against the first
    layer's input_dim / connect."""
    from types import SimpleNamespace
    from dgp_amd.pathwalk import connect_cols, connect_split
    node = lambda c: SimpleNamespace(connect=None if c is None else np.array(c))
    internal, external = np.array([0, 2, 1]), np.array([4, 3])
    head, alone = SimpleNamespace(input_dim=internal, connect=external), SimpleNamespace(input_dim=internal, connect=None)
    same = lambda got, want: all(np.array_equal(a, np.asarray(b, dtype=int)) for a, b in zip(got, want)) and len(got) == 2
    for last in (False, True):
        for shared in (False, True):
            assert same(connect_cols(node(None), last, shared, 3, head), ([], []))
        assert same(connect_cols(node([4, 1]), last, True, 3, head), ([4, 1], []))
    assert same(connect_cols(node([1, 3, 4]), False, False, 3, head), ([1], [0, 1]))
    assert same(connect_cols(node([0, 1]), False, False, 3, alone), ([0, 1], []))
    assert same(connect_cols(node([2, 3]), True, False, 3, head), ([1], [1]))
    assert same(connect_cols(node([1, 0]), True, False, 3, alone), ([2, 0], []))
    for c, last in (([1, 3, 4], False), ([2, 3], True)):
        assert same(connect_cols(node(c), last, False, 3, head), connect_split(np.array(c), last, 3, internal, external))
