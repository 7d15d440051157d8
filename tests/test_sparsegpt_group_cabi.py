"""CPU: `ecoflap_sparsegpt_matrix_group` refuses bad arguments — of ANY member — before it touches a
device (no GPU here: a call that got past its checks would fail otherwise), with the single entry's
error codes, and its workspace query covers the stacked layout."""
import ctypes

import pytest

EDTYPE, ENULL, ESIZE, EWORKSPACE = -1, -2, -3, -6
F16 = 1
P = ctypes.c_void_p
COLS = 200                      # two column blocks: 128 + 72


@pytest.fixture(scope="module")
def lib():
    from ecoflap_amd import hip
    return hip.load_library()


def members(rows=(8, 5, 1), weights=(0x10000, 0x20000, 0x30000), ranks=((100, 50), (60, 30), (10, 7))):
    from ecoflap_amd import hip
    items = (hip.SgptGroupItem * max(len(rows), 1))()
    keep = []
    for i in range(len(rows)):
        it = items[i]
        it.w, it.rows = weights[i], rows[i]
        if ranks is not None and ranks[i] is not None:
            keep.append((ctypes.c_int64 * len(ranks[i]))(*ranks[i]))
            it.ranks_host = ctypes.cast(keep[-1], ctypes.c_void_p)
    return items, keep


def group(lib, items=None, n=None, dtype=F16, cols=COLS, hinv=0x2000, ldh=COLS, dead=None, blocksize=128,
          pn=0, pm=0, ws=0x4000, ws_bytes=None, **member_args):
    keep = None
    if items is None:
        items, keep = members(**member_args)
        if n is None:
            n = len(member_args.get("rows", (8, 5, 1)))
    if ws_bytes is None:
        ws_bytes = lib.ecoflap_sparsegpt_matrix_group_workspace_bytes(ctypes.byref(items), n, cols)
    rc = lib.ecoflap_sparsegpt_matrix_group(ctypes.byref(items), n, dtype, cols, P(hinv), ldh, P(dead), blocksize,
                                            pn, pm, P(ws), ws_bytes, None, None)
    del keep
    return rc


def test_group_argument_errors(lib):
    assert group(lib, weights=(0x10000, None, 0x30000)) == ENULL                  # a member without a weight
    assert group(lib, hinv=None) == ENULL
    assert group(lib, ws=None) == ENULL
    assert group(lib, ranks=((100, 50), None, (10, 7))) == ENULL             # thresholded: every member's ranks
    assert lib.ecoflap_sparsegpt_matrix_group(None, 2, F16, COLS, P(0x2000), COLS, None, 128, 0, 0, P(0x4000),
                                              1 << 30, None, None) == ENULL
    items, keep = members()
    assert group(lib, items=items, n=0, ws_bytes=1 << 30) == ESIZE           # no members
    nine, keep9 = members(rows=(4,) * 9, weights=(0x10000,) * 9, ranks=((1, 1),) * 9)
    assert group(lib, items=nine, n=9, ws_bytes=1 << 30) == ESIZE            # more than 8
    assert group(lib, items=nine, n=8, ws_bytes=1) == EWORKSPACE             # 8 pass the size checks
    assert group(lib, ranks=((100, 50), (60, -1), (10, 7))) == ESIZE         # a bad rank in the second member only
    assert group(lib, ranks=((100, 50), (5 * 128, 30), (10, 7))) == ESIZE    # past ITS block's last element
    assert group(lib, ranks=((100, 50), (60, 30), (128, 7))) == ESIZE        # the one-row member's limit is 127
    # (fine for the member of 8 rows — limits are per member: the call gets as far as the workspace check)
    assert group(lib, ranks=((7 * 128, 50), (60, 30), (10, 7)), ws_bytes=1) == EWORKSPACE
    assert group(lib, rows=(8, 0, 1)) == ESIZE
    assert group(lib, ldh=COLS - 1) == ESIZE
    assert group(lib, blocksize=129) == ESIZE
    assert group(lib, blocksize=0) == ESIZE
    assert group(lib, pn=3, pm=2, ranks=None) == ESIZE                       # n:m with n > m
    assert group(lib, pn=0, pm=4) == ESIZE
    need = lib.ecoflap_sparsegpt_matrix_group_workspace_bytes(ctypes.byref(items), 3, COLS)
    assert group(lib, ws_bytes=need - 1) == EWORKSPACE
    assert group(lib, dtype=7) == EDTYPE


@pytest.mark.parametrize("rows,cols", [((1,), 1), ((130, 33, 1), 328), ((256, 256, 256), 256),
                                       ((4096, 4096, 4096), 4096), ((11008, 11008), 4096)])
def test_workspace_covers_the_stacked_layout(lib, rows, cols):
    from ecoflap_amd import hip
    items = (hip.SgptGroupItem * len(rows))()
    for it, r in zip(items, rows):
        it.w, it.rows = 0x1000, r
    got = lib.ecoflap_sparsegpt_matrix_group_workspace_bytes(ctypes.byref(items), len(rows), cols)
    total = sum(rows)
    assert got >= total * cols * 4 + total * 128 * 4 + len(rows) * 3 * 2048 * 4     # copy, Err, a state per member
    # and not more than that with every member on a 4-row boundary and 256-byte sections
    padded = sum((r + 3) // 4 * 4 for r in rows)
    assert got <= padded * cols * 4 + padded * 128 * 4 + len(rows) * 3 * 2048 * 4 + 3 * 256


@pytest.mark.parametrize("rows,cols", [(1, 1), (130, 328), (768, 3072), (4096, 4096)])
def test_one_member_needs_at_least_the_single_entrys_workspace(lib, rows, cols):
    from ecoflap_amd import hip
    items = (hip.SgptGroupItem * 1)()
    items[0].w, items[0].rows = 0x1000, rows
    assert (lib.ecoflap_sparsegpt_matrix_group_workspace_bytes(ctypes.byref(items), 1, cols)
            >= lib.ecoflap_sparsegpt_matrix_workspace_bytes(rows, cols))


def test_workspace_query_refuses_what_the_entry_refuses(lib):
    from ecoflap_amd import hip
    items = (hip.SgptGroupItem * 9)()
    for it in items:
        it.w, it.rows = 0x1000, 4
    q = lib.ecoflap_sparsegpt_matrix_group_workspace_bytes
    assert q(ctypes.byref(items), 0, 8) == 0 and q(ctypes.byref(items), 9, 8) == 0
    assert q(None, 2, 8) == 0 and q(ctypes.byref(items), 2, 0) == 0
    items[1].rows = 0
    assert q(ctypes.byref(items), 2, 8) == 0


def test_python_bindings_exist():
    from ecoflap_amd import hip
    assert "ecoflap_sparsegpt_matrix_group" in hip.EXPORTS
    assert "ecoflap_sparsegpt_matrix_group_workspace_bytes" in hip.EXPORTS
    assert callable(hip.HipKernels.sparsegpt_matrix_group)
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    assert callable(SparseGPT.sweep_group)
