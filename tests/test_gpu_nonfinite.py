"""GPU test of the finiteness verdict's kernel (csrc/range.hip, mode PDSE_RANGE_NONFINITE) through ``_lib.launch``: out[r][0]
grows by the number of Inf / NaN elements of row r's fp32 tensor, counted on the host from the same bits (exact integers)."""
import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 1031, 4096 + 7)
OFFSETS = (0, 1, 2, 3)                       # floats from the allocation (512-byte aligned): the scalar head is (4 - off) % 4 elements
NAN, PINF, NINF, NEG_NAN_PAYLOAD = 0x7fc00000, 0x7f800000, 0xff800000, 0xffc12345
BAD = (NAN, PINF, NINF, NEG_NAN_PAYLOAD)
# finite values that must not count: +-FLT_MAX, 65504, 2^15, the smallest and largest subnormal of either sign, +-0
FINE = (0x7f7fffff, 0xff7fffff, 0x477fe000, 0x47000000, 0x00000001, 0x807fffff, 0x007fffff, 0x00000000, 0x80000000)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _host_count(bits):
    return int(((bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).sum())


def _bits(rng, n, off, nrandom):
    """n fp32 bit patterns: finite random values of every exponent, the FINE specials, and non-finite values at index 0, n - 1,
    on both sides of the head / body boundary, inside the tail and at ``nrandom`` random places."""
    u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[(u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)] &= np.uint32(0xbfffffff)      # random Inf / NaN patterns made finite
    for j, f in enumerate(FINE):
        if n:
            u[(5 * j + 2) % n] = f
    head = min(n, (4 - off) % 4)
    tail = (n - head) % 4
    spots = [0, n - 1, head - 1, head, head + 1, n - tail, n - 2] + rng.integers(0, max(n, 1), nrandom).tolist()
    for j, i in enumerate(spots):
        if 0 <= i < n:
            u[i] = BAD[j % 4]
    return u


class _View:
    """Bit patterns as fp32 device memory that starts ``off`` floats into its allocation: (ptr, n) of a row.  The pointer is
    computed from the allocation (an empty torch view has none), so an n = 0 row has a valid one too."""

    def __init__(self, bits, off):
        self.buf = torch.zeros(bits.size + off + 8, dtype=torch.int32, device=DEV)
        self.buf[off:off + bits.size].copy_(torch.from_numpy(bits.view(np.int32)))
        self.ptr, self.n = self.buf.data_ptr() + 4 * off, int(bits.size)
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (4 * off) % 16


def _view(bits, off, keep):
    keep.append(_View(bits, off))
    return keep[-1]


def _launch(L, tensors, out, keep, blocks=None):
    RA = pkg("rangeaudit")
    rows = []
    for t in tensors:
        r = L.RangeRow()                     # pointer and length: every other field stays zero
        r.ptr, r.n = t.ptr, t.n
        rows.append(r)
    dev = torch.from_numpy(RA.table_of(rows)).to(DEV)
    keep.append(dev)
    d = L.RangeDesc()
    d.rows, d.nrows, d.out, d.out_rows, d.mode = dev.data_ptr(), len(rows), out.data_ptr(), out.shape[0], L.RANGE_NONFINITE
    d.blocks = RA.work_blocks(rows) if blocks is None else blocks
    L.launch(d)


def _table(out):
    return out.cpu().numpy().view(np.uint32).astype(np.int64)


PATTERN = 0x5a5a0000


def _pattern(rows):
    return (torch.arange(rows * 32, dtype=torch.int32, device=DEV) + PATTERN).reshape(rows, 32)


@pytest.fixture(scope="module")
def cases(L):
    """Every (n, offset) pair as one tensor, with its host count; shared by the tests below and never written again."""
    rng = np.random.default_rng(2024)
    keep, out = [], []
    for n in SIZES:
        for off in OFFSETS:
            bits = _bits(rng, n, off, 3000 if n > 4096 else (n // 8))
            out.append((n, off, _view(bits, off, keep), _host_count(bits)))
    big = _bits(rng, 3 * 2048 * 4 + 5, 1, 5000)                      # more vectors than one workgroup's share: several workgroups
    out.append((big.size, 1, _view(big, 1, keep), _host_count(big)))
    assert sum(c for *_, c in out) > 8000 and any(c == 0 for n, _, _, c in out if n == 0)
    return out, keep


def test_counts_equal_the_host_for_every_size_and_alignment(L, cases):
    """One launch over all 41 rows (different n in one table), then every row alone: column 0 is the host's count, bins 1 .. 31
    keep the pattern the table was filled with, rows beyond the table's are untouched."""
    rows, keep = cases
    tens, want = [t for _, _, t, _ in rows], [c for *_, c in rows]
    out = _pattern(len(rows) + 1)
    before = _table(out)
    _launch(L, tens, out, keep)
    got = _table(out)
    assert (got[:len(rows), 0] - before[:len(rows), 0]).tolist() == want
    assert np.array_equal(got[:, 1:], before[:, 1:]) and np.array_equal(got[len(rows)], before[len(rows)])
    for n, off, t, c in rows:
        one = torch.zeros(1, 32, dtype=torch.int32, device=DEV)
        _launch(L, [t], one, keep)
        assert _table(one)[0].tolist() == [c] + [0] * 31, (n, off)


@pytest.mark.parametrize("blocks", [2, 3, 7])
def test_more_workgroups_than_work_and_grid_stride(L, cases, blocks):
    """The grid is the caller's: with more workgroups than a row has vectors for (most return at once) and with fewer than the
    largest row needs (grid-stride) the counts are the same."""
    rows, keep = cases
    pick = [r for r in rows if r[0] in (0, 5, 257, 1031, 4103)] + [rows[-1]]
    out = torch.zeros(len(pick), 32, dtype=torch.int32, device=DEV)
    _launch(L, [t for _, _, t, _ in pick], out, keep, blocks=blocks)
    assert _table(out)[:, 0].tolist() == [c for *_, c in pick] and not _table(out)[:, 1:].any()


def test_two_and_three_rows_and_a_second_launch_adds(L, cases):
    rows, keep = cases
    by = {(n, off): (t, c) for n, off, t, c in rows}
    for pick in ([(257, 1), (4103, 3)], [(1031, 2), (3, 0), (4103, 0)]):
        tens, want = [by[k][0] for k in pick], [by[k][1] for k in pick]
        out = _pattern(len(pick))
        before = _table(out)
        _launch(L, tens, out, keep)
        _launch(L, tens, out, keep)                                  # no clear in between: the counts add up
        got = _table(out)
        assert (got[:, 0] - before[:, 0]).tolist() == [2 * w for w in want] and all(w > 0 for w in want)
        assert np.array_equal(got[:, 1:], before[:, 1:])
    # the operator's clear (mode 0) is what a plan starts from
    d = L.RangeDesc()
    d.out, d.out_rows, d.mode, d.blocks = out.data_ptr(), out.shape[0], L.RANGE_CLEAR, 1
    L.launch(d)
    assert not _table(out).any()


def test_all_finite_tensors_leave_the_table_untouched(L):
    """Finite values of every kind - the FINE specials among them, at every alignment - add nothing: the table keeps its bits."""
    rng = np.random.default_rng(7)
    keep, tens = [], []
    for off in OFFSETS:
        u = rng.integers(0, 2 ** 32, 4096 + 7, dtype=np.uint64).astype(np.uint32)
        u[(u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)] &= np.uint32(0xbfffffff)
        u[:len(FINE)] = FINE
        u[-len(FINE):] = FINE
        assert _host_count(u) == 0
        tens.append(_view(u, off, keep))
    out = _pattern(len(tens))
    before = _table(out)
    _launch(L, tens, out, keep)
    assert np.array_equal(_table(out), before)


def test_rows_are_validated_before_the_launch(L):
    t = torch.zeros(16, device=DEV)
    out = torch.zeros(1, 32, dtype=torch.int32, device=DEV)
    RA = pkg("rangeaudit")
    for field, val, msg in (("ptr", None, "null tensor"), ("n", -1, "n < 0"), ("ptr", t.data_ptr() + 2, "aligned to 4")):
        r = L.RangeRow()
        r.ptr, r.n = t.data_ptr(), t.numel()
        setattr(r, field, val)
        dev = torch.from_numpy(RA.table_of([r])).to(DEV)
        d = L.RangeDesc()
        d.rows, d.nrows, d.out, d.out_rows, d.mode, d.blocks = dev.data_ptr(), 1, out.data_ptr(), 1, L.RANGE_NONFINITE, 1
        with pytest.raises(L.PdseError, match=msg):
            L.launch(d)
    torch.cuda.synchronize()
    assert not _table(out).any()
