"""CPU: `ecoflap_sparsegpt_trailing` and `ecoflap_sparsegpt_matrix` refuse bad arguments before
they touch a device (no GPU here: a call that got past its checks would fail otherwise), with the
library's error codes, and the workspace query covers what the entry keeps in it."""
import ctypes

import pytest

ENULL, ESIZE, EWORKSPACE = -2, -3, -6
F16 = 1
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from ecoflap_amd import hip
    return hip.load_library()


def trailing(lib, W=0x1000, rows=8, cols=256, ldw=256, err=0x2000, hinv=0x3000, ldh=256, i1=0, count=128, j0=128):
    return lib.ecoflap_sparsegpt_trailing(P(W), rows, cols, ldw, P(err), P(hinv), ldh, i1, count, j0, None)


def test_trailing_argument_errors(lib):
    assert trailing(lib, W=None) == ENULL
    assert trailing(lib, err=None) == ENULL
    assert trailing(lib, hinv=None) == ENULL
    assert trailing(lib, count=129) == ESIZE
    assert trailing(lib, count=0) == ESIZE
    assert trailing(lib, rows=0) == ESIZE
    assert trailing(lib, j0=257) == ESIZE           # past the last column
    assert trailing(lib, ldw=255) == ESIZE
    assert trailing(lib, ldh=255) == ESIZE
    assert trailing(lib, i1=-1) == ESIZE
    assert trailing(lib, j0=256) == 0               # no columns remain: nothing is launched


def matrix(lib, w=0x1000, rows=8, cols=200, hinv=0x2000, ldh=200, dead=None, blocksize=128, ranks=(100, 50),
           n=0, m=0, ws=0x4000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ecoflap_sparsegpt_matrix_workspace_bytes(rows, cols)
    ranks_a = None if ranks is None else (ctypes.c_int64 * len(ranks))(*ranks)
    return lib.ecoflap_sparsegpt_matrix(P(w), F16, rows, cols, P(hinv), ldh, P(dead), blocksize, ranks_a, n, m,
                                        P(ws), ws_bytes, None)


def test_matrix_argument_errors(lib):
    assert matrix(lib, w=None) == ENULL
    assert matrix(lib, hinv=None) == ENULL
    assert matrix(lib, ws=None) == ENULL
    assert matrix(lib, ranks=None) == ENULL                      # thresholded: the ranks are needed
    assert matrix(lib, blocksize=129) == ESIZE                   # count > 128
    assert matrix(lib, blocksize=0) == ESIZE
    assert matrix(lib, ranks=(100, -1)) == ESIZE                 # a negative rank
    assert matrix(lib, ranks=(8 * 128, 50)) == ESIZE             # a rank past the block's last element
    assert matrix(lib, ldh=199) == ESIZE
    assert matrix(lib, n=3, m=2, ranks=None) == ESIZE            # n:m with n > m
    assert matrix(lib, ws_bytes=lib.ecoflap_sparsegpt_matrix_workspace_bytes(8, 200) - 1) == EWORKSPACE
    assert lib.ecoflap_sparsegpt_matrix(P(0x1000), 7, 8, 200, P(0x2000), 200, None, 128,
                                        (ctypes.c_int64 * 2)(1, 1), 0, 0, P(0x4000), 1 << 20, None) == -1   # dtype


@pytest.mark.parametrize("rows,cols", [(1, 1), (130, 328), (768, 3072), (3072, 768)])
def test_workspace_covers_the_working_copy_and_err(lib, rows, cols):
    assert lib.ecoflap_sparsegpt_matrix_workspace_bytes(rows, cols) >= rows * cols * 4 + rows * 128 * 4


def test_python_bindings_exist():
    from ecoflap_amd import hip
    assert "ecoflap_sparsegpt_trailing" in hip.EXPORTS and "ecoflap_sparsegpt_matrix" in hip.EXPORTS
    assert callable(hip.HipKernels.sparsegpt_trailing) and callable(hip.HipKernels.sparsegpt_matrix)
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    assert SparseGPT.whole_matrix_sweep is False
