"""The tile heights of the bf16 ping-pong GEMM (pick_tile_rows) on the host, through the pure hook fmi_gemm_tile_rows: which rows of a
problem go to 256-row tiles and which to 192-row tiles, on 256 compute units unless a case says otherwise.  No GPU: the hook schedules on the CU
count it is given."""
import ctypes as C

import pytest

from diffusion_rs_amd import _lib as L

CUS = 256
AUTO, TALL, SHORT, MIXED = 0, 256, 192, 448


def split(Ms, Ns, mode=AUTO, q8=0, cus=CUS):
    lib = L.load()
    n = len(Ms)
    arr = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
    n256, n192, ts, ss, q = arr([0] * n), arr([0] * n), arr([0] * (n + 1)), arr([0] * (n + 1)), C.c_int(0)
    L.check(lib.fmi_gemm_tile_rows(arr(Ms), arr(Ns), n, cus, q8, mode, n256, n192, ts, ss, C.byref(q)), lib)
    return list(n256), list(n192), list(ts), list(ss), q.value


def covered(M, a, b):
    """Rows the tiles cover, the last one clamped to M: every row exactly once."""
    tall = min(a * 256, M)
    if b == 0:
        return a == -(-M // 256)
    return a * 256 < M and (b - 1) * 192 < M - tall <= b * 192


def test_mlp_in_is_cut_12_plus_8():
    a, b, _, _, q = split([4608], [12288])
    assert (a, b) == ([12], [8])
    assert q == 14  # 3.5 rounds instead of 4


def test_grouped_qkv_is_cut_below_three_rounds():
    a, b, _, _, q = split([4096, 512], [9216, 9216])
    assert sum(b) > 0 and q < 12
    assert all(covered(M, x, y) for M, x, y in zip((4096, 512), a, b))
    assert split([4096, 512], [9216, 9216], mode=TALL)[4] == 12


@pytest.mark.parametrize("Ms,Ns,q8", [([4608], [3072], 0), ([4608], [21504], 0), ([256], [12288], 0), ([256], [512], 0), ([200], [3072], 0),
                                      ([4608], [12288], 1), ([4608], [12288], 2), ([4096, 512], [9216, 9216], 1)])
def test_all_tall_where_nothing_is_gained_and_for_8_bit_kinds(Ms, Ns, q8):
    a, b, _, _, _ = split(Ms, Ns, q8=q8)
    assert b == [0] * len(Ms) and a == [-(-M // 256) for M in Ms]


def test_8_bit_kinds_ignore_a_forced_height():
    for mode in (SHORT, MIXED):
        assert split([4608], [12288], mode=mode, q8=2)[1] == [0]


@pytest.mark.parametrize("mode", [AUTO, TALL, SHORT, MIXED])
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_rows_sum_to_m_and_tall_tiles_come_first(mode, cus):
    groups = [([M], [N]) for M in (100, 192, 256, 400, 448, 640, 703, 704, 4096, 4608, 4600, 9216) for N in (512, 3072, 9216, 12288)]
    groups += [([4096, 512], [9216, 9216]), ([448, 192], [512, 512]), ([4608, 300, 77], [12288, 260, 512]), ([1000] * 8, [1024] * 8)]
    for Ms, Ns in groups:
        a, b, ts, ss, q = split(Ms, Ns, mode=mode, cus=cus)
        assert all(covered(M, x, y) for M, x, y in zip(Ms, a, b)), (Ms, Ns, a, b)
        cols = [-(-N // 256) for N in Ns]
        # the launch order: the tall regions of all problems, contiguous from 0, then the short regions, contiguous to the grid's end
        assert ts[0] == 0 and all(ts[i + 1] - ts[i] == a[i] * cols[i] for i in range(len(Ms)))
        assert ss[0] == ts[-1] and all(ss[i + 1] - ss[i] == b[i] * cols[i] for i in range(len(Ms)))
        assert max(ts) <= min(ss)
        assert q > 0
        if mode == AUTO:  # never worse than all tall in its own model, and a cut only for a quarter round or more
            q_tall = split(Ms, Ns, mode=TALL, cus=cus)[4]
            assert q <= q_tall and (sum(b) == 0 or q <= q_tall - 1)


def test_forced_heights():
    assert split([400], [512], mode=SHORT)[:2] == ([0], [3])    # 192 + 192 + 16
    assert split([448], [512], mode=MIXED)[:2] == ([1], [1])
    assert split([640], [512], mode=MIXED)[:2] == ([1], [2])
    assert split([192], [512], mode=MIXED)[:2] == ([0], [1])
    assert split([100], [512], mode=MIXED)[:2] == ([0], [1])
    assert split([448, 192], [512, 512], mode=MIXED)[:2] == ([1, 0], [1, 1])


def test_setter_accepts_the_four_settings_only():
    lib = L.load()
    try:
        for v in (256, 192, 448, 0):
            assert lib.fmi_set_gemm_rows(v) == 0
        assert lib.fmi_set_gemm_rows(128) == L.ERR_INVALID and b"set_gemm_rows" in lib.fmi_last_error()
    finally:
        lib.fmi_set_gemm_rows(0)
