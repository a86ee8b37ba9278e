"""sslam_batch_marginals, the part that needs no device: the symbol is exported and declared to ctypes, a NULL handle is refused, and the
Python wrappers reject malformed requests before they reach the library."""
import ctypes as C

import numpy as np
import pytest


def test_symbol_is_exported_and_bound(hip_lib):
    fn = hip_lib.sslam_batch_marginals
    assert fn.restype is C.c_int and len(fn.argtypes) == 4


def test_null_handle_is_invalid(hip_lib):
    req = np.array([0, 1, 1], np.int32)
    out = np.full(36, -7.0)
    rc = hip_lib.sslam_batch_marginals(None, req.ctypes.data_as(C.POINTER(C.c_int32)), 1, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and b"null" in hip_lib.sslam_last_error()
    assert np.all(out == -7.0)
    assert hip_lib.sslam_batch_marginals(None, None, 0, None) == -1      # the handle is checked before n == 0


class _NoCalls:
    """stands in for the loaded library: any entry point a wrapper reaches for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its arguments")


def _unbuilt_batch(n_graphs):
    from semantic_slam_amd import GraphBatch
    B = GraphBatch.__new__(GraphBatch)      # no device here: a batch object without a handle, enough for the argument checks
    B._lib, B._h, B.graphs = _NoCalls(), None, [object()] * n_graphs
    return B


@pytest.mark.parametrize("bad,exc", [
    ([(0, 1)], ValueError),                 # a pair instead of a triple
    ([(0, 1, 2, 3)], ValueError),
    ([5], ValueError),                      # not a sequence
    ([(0, 1.5, 1)], TypeError),             # a vertex id that is no integer
    ([(0, "1", 1)], TypeError),
    ([(True, 1, 1)], TypeError),
    ([(0, 1, 1), (2, 0, 0)], IndexError),   # graph index past the batch
    ([(-1, 0, 0)], IndexError),
])
def test_wrappers_reject_malformed_requests_before_any_c_call(hip_lib, bad, exc):
    B = _unbuilt_batch(2)
    with pytest.raises(exc):
        B.marginals(bad)


def test_landmark_marginals_wants_one_list_per_graph(hip_lib):
    B = _unbuilt_batch(2)
    with pytest.raises(ValueError):
        B.landmark_marginals([[1, 2]])
    with pytest.raises(TypeError):
        B.landmark_marginals([[1, 2], [0.5]])
