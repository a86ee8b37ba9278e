"""sslam_batch_gate / sslam_graph_gate, the part that needs no device: the symbols are exported and declared to ctypes, a NULL handle is
refused with the outputs untouched, and the Python wrappers reject malformed candidates before they reach the library."""
import ctypes as C

import numpy as np
import pytest


def test_symbols_are_exported_and_bound(hip_lib):
    for name in ("sslam_batch_gate", "sslam_graph_gate"):
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 8


@pytest.mark.parametrize("name,width", [("sslam_batch_gate", 4), ("sslam_graph_gate", 3)])
def test_null_handle_is_invalid(hip_lib, name, width):
    fn = getattr(hip_lib, name)
    dp = C.POINTER(C.c_double)
    cand = np.array([0, 0, 1, 2][4 - width:], np.int32)
    z = np.array([1.0, 0, 0, 0, 0, 0, 1])
    outs = [np.full(1, -7.0), np.full(6, -7.0), np.full(36, -7.0)]
    rc = fn(None, cand.ctypes.data_as(C.POINTER(C.c_int32)), z.ctypes.data_as(dp), None, 1, *[o.ctypes.data_as(dp) for o in outs])
    assert rc == -1 and b"null" in hip_lib.sslam_last_error()
    assert all(np.all(o == -7.0) for o in outs)
    assert fn(None, None, None, None, 0, None, None, None) == -1      # the handle is checked before n == 0


class _NoCalls:
    """stands in for the loaded library: any entry point a wrapper reaches for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its arguments")


def _unbuilt_batch(n_graphs):
    from semantic_slam_amd import GraphBatch
    B = GraphBatch.__new__(GraphBatch)      # no device here: a batch object without a handle, enough for the argument checks
    B._lib, B._h, B.graphs = _NoCalls(), None, [object()] * n_graphs
    return B


Z7, Z3 = [0.5, 0, 0, 0, 0, 0, 1.0], [1.0, 2.0, 3.0]


@pytest.mark.parametrize("bad,exc", [
    ([(0, "se3", 1, 2, Z7)], ValueError),                       # five entries instead of six
    ([(0, "se3", 1, 2, Z7, None, 1)], ValueError),
    ([5], ValueError),                                          # not a sequence
    ([(0, "se3", 1.5, 2, Z7, None)], TypeError),                # a vertex id that is no integer
    ([(0, "se3", 1, "2", Z7, None)], TypeError),
    ([(True, "se3", 1, 2, Z7, None)], TypeError),
    ([(0, "se3", 1, 2, Z7, None), (2, "se3", 1, 2, Z7, None)], IndexError),   # graph index past the batch
    ([(-1, "se3", 1, 2, Z7, None)], IndexError),
    ([(0, "plane", 1, 2, Z7, None)], ValueError),               # kind name
    ([(0, 0, 1, 2, Z7, None)], ValueError),
    ([(0, "se3", 1, 2, Z3, None)], ValueError),                 # z shapes: 7 for "se3", 3 for "point"
    ([(0, "point", 1, 2, Z7, None)], ValueError),
    ([(0, "se3", 1, 2, Z7, np.eye(3))], ValueError),            # info shapes: 6x6 for "se3", 3x3 for "point"
    ([(0, "point", 1, 2, Z3, np.eye(6))], ValueError),
    ([(0, "point", 1, 2, Z3, np.ones(9))], ValueError),
])
def test_wrapper_rejects_malformed_candidates_before_any_c_call(hip_lib, bad, exc):
    B = _unbuilt_batch(2)
    with pytest.raises(exc):
        B.gate(bad)
    with pytest.raises(exc):
        B.gate(bad, return_cov=True)


def test_no_candidates_no_call(hip_lib):
    B = _unbuilt_batch(2)
    assert B.gate([]).shape == (0,)
    d2, e, S = B.gate([], return_cov=True)
    assert d2.shape == (0,) and e == [] and S == []


def test_cpp_shim_gate_compiles_and_checks_its_arguments(hip_lib, tmp_path):
    """tests/shim_gate_check.cpp: without a GPU it stops after the host-side checks (a candidate from a vertex to itself is refused)"""
    import os
    import subprocess
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_gate")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_gate_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shim gate ok" in out.stdout
