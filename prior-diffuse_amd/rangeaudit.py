"""Range audit of the f16x2 window: the host side of csrc/range.hip (include/pdse.h: pdse_range_desc).

``make_row`` turns an entry of a plan builder's ``audited()`` list into a row of an accumulate launch's table; ``RangeReport`` reads the
histogram table the launches filled.

Why the two verdicts are what they are (they follow from the format, they are not tuned).  An f16x2 operand is the fp32 value
x, scaled by a power of two, carried as hi = RN16(x) and lo = RN16(x - hi).  hi has 11 significand bits, so for hi in binade
E (2^E <= |hi| < 2^(E+1)) the remainder |x - hi| is at most half a unit of hi's last place, 2^(E-11).  lo rounds that
remainder to 11 more bits: while lo is a normal fp16 the second rounding errs by at most 2^-11 of the remainder, 2^(E-23)
<= 2^-23 |x|; where lo is subnormal (remainder under 2^-14) it errs by at most half the subnormal spacing, 2^-25, absolute.
Both are within 2^-23 |x| exactly when 2^-25 <= 2^-23 2^E, i.e. E >= -2: from hi's exponent -2 up the pair carries its
11 + 11 bits and |x - hi - lo| <= 2^-23 |x|; under it the bound is the absolute 2^-25 in scaled units (2^-29 in true scale with
PDSE_F16_ACT_EXP = 4) whatever the size of x, so the relative error grows as x shrinks.  Hence, on the histogram of hi's binade:

* a tensor is ``below`` when its largest non-zero scaled magnitude is under 2^-2 (no bin from RANGE_BIN_FULL up is occupied,
  some bin under it is): not one of its elements is carried at full precision.  A tensor with SOME small elements is not
  below - small addends next to large ones are covered by the absolute bound, see include/pdse.h - and ``below_frac`` reports
  their share;
* a tensor is ``above`` when bin 31 is occupied: a scaled magnitude reached 2^15, the last fp16 binade, where hi turns into
  an infinity at 65520 (or the value was not finite to begin with).
A tensor of zeros is neither."""
import numpy as np

from . import _lib as L


class ReportRow:
    """One (marked range, tensor) of a report: ``hist`` are the 32 counters of csrc/range.hip (``_lib.RANGE_BINADE``)."""

    def __init__(self, name, range_, hist):
        hist = [int(v) for v in hist]
        if len(hist) != L.RANGE_BINS:
            raise ValueError("a histogram has %d bins" % L.RANGE_BINS)
        self.name, self.range, self.hist = name, range_, hist
        self.count = sum(hist)
        nz = [b for b in range(1, L.RANGE_BINS) if hist[b]]
        self.nonzero = sum(hist[1:])
        # exponent of the lower edge of the highest occupied binade in scaled units (-inf: all under 2^-14; None: all zero)
        self.max_binade = L.RANGE_BINADE[nz[-1]] if nz else None
        self.below_frac = sum(hist[1:L.RANGE_BIN_FULL]) / self.nonzero if self.nonzero else 0.0
        self.below = bool(nz) and nz[-1] < L.RANGE_BIN_FULL
        self.above = hist[L.RANGE_BIN_TOP] > 0

    @property
    def ok(self):
        return not (self.below or self.above)

    def __repr__(self):
        return "ReportRow(%r, %r, count=%d, max_binade=%r, below_frac=%.3g%s%s)" % (
            self.name, self.range, self.count, self.max_binade, self.below_frac, ", below" if self.below else "",
            ", above" if self.above else "")


class RangeReport:
    """What ``SamplerPipeline.range_report()`` returns: ``rows`` in plan order (per marked range, per audited tensor)."""

    def __init__(self, rows):
        self.rows = list(rows)

    @property
    def ok(self):
        return all(r.ok for r in self.rows)

    def below(self):
        return [r for r in self.rows if r.below]

    def above(self):
        return [r for r in self.rows if r.above]

    def worst(self):
        """The row that is furthest from the window: the first ``above`` row, else the first ``below`` row, else the row with
        the largest share of elements under the full-precision edge (None for an empty report)."""
        for pick in (self.above(), self.below()):
            if pick:
                return pick[0]
        return max(self.rows, key=lambda r: r.below_frac) if self.rows else None

    def __len__(self):
        return len(self.rows)

    def __iter__(self):
        return iter(self.rows)

    def table(self):
        """Printable table: one line per row; magnitudes are in true scale (scaled binade less PDSE_F16_ACT_EXP)."""
        from .packing import F16_ACT_EXP

        lines = ["%-8s %-24s %12s %10s %11s  %s" % ("range", "tensor", "elements", "max |x|", "under 2^%d" % (L.RANGE_BINADE[L.RANGE_BIN_FULL] - F16_ACT_EXP), "verdict")]
        for r in self.rows:
            if r.max_binade is None:
                top = "0"
            elif r.max_binade == float("-inf"):
                top = "< 2^%d" % (-14 - F16_ACT_EXP)
            else:
                top = "%s2^%d" % (">= " if r.above else "< ", r.max_binade - F16_ACT_EXP + (0 if r.above else 1))
            lines.append("%-8s %-24s %12d %10s %10.2f%%  %s" % (r.range, r.name, r.count, top, 100.0 * r.below_frac,
                                                               "ABOVE" if r.above else ("BELOW" if r.below else "ok")))
        return "\n".join(lines)

    __str__ = table


def make_row(tensor, kind, exp, layout, out_row):
    """One pdse_range_row of an ``audited()`` entry."""
    r = L.RangeRow()
    r.kind, r.exp, r.out_row = int(kind), int(exp), int(out_row)
    if kind == L.RANGE_F32:
        if not tensor.is_contiguous() or tensor.element_size() != 4:
            raise ValueError("a RANGE_F32 tensor is a contiguous fp32 tensor")
        r.ptr, r.n = tensor.data_ptr(), tensor.numel()
    elif kind == L.RANGE_F16HI:
        n0, n1, n2, n3 = (int(v) for v in layout["dims"])
        r.ptr = tensor.data_ptr() + 2 * int(layout["off"])
        r.n0, r.n1, r.n2, r.n3 = n0, n1, n2, n3
        r.s0, r.s1, r.s2 = (int(v) for v in layout["strides"])
        r.i0, r.par_half = int(layout["i0"]), int(layout["par_half"])
        r.n = 8 * n0 * n1 * n2 * n3
        # the last vector the walk can reach must lie inside the tensor
        if min(n0, n1, n2, n3) < 1:
            raise ValueError("empty layout")
        i = np.arange(r.i0, r.i0 + n3)
        pos = int(((i & 1) * r.par_half + (i >> 1) if r.par_half else i).max())
        last = int(layout["off"]) + (n0 - 1) * r.s0 + (n1 - 1) * r.s1 + (n2 - 1) * r.s2 + 8 * pos + 8
        if tensor.element_size() != 2 or last > tensor.numel():
            raise ValueError("the layout does not fit the tensor")
    else:
        raise ValueError("unknown element kind %r" % (kind,))
    return r


def work_blocks(rows, per_block=256 * 8, most=1024):
    """Workgroups per row (grid x) for a table: enough for the largest row at eight 16-byte loads per lane, at most four per CU
    (measured best on the largest tensors of the B = 32, T = 401 plan: profiles/range_audit_timing.txt)."""
    vec = max((r.n + 3) // 4 if r.kind == L.RANGE_F32 else r.n // 8 for r in rows)
    return int(min(most, max(1, -(-vec // per_block))))


def table_of(rows):
    """The bytes (numpy uint8) of the device table of a list of ``_lib.RangeRow``."""
    arr = (L.RangeRow * len(rows))(*rows)
    return np.frombuffer(arr, dtype=np.uint8).copy()


def histogram(values, exp=0):
    """Host counterpart of csrc/range.hip for tests and tools: the 32 counters of float values scaled by 2^exp (float64
    arithmetic; reads the exported table, not the kernel's formula)."""
    v = np.abs(np.asarray(values, np.float64).reshape(-1))
    hist = np.zeros(L.RANGE_BINS, np.int64)
    bad = ~np.isfinite(v)
    hist[L.RANGE_BIN_TOP] += int(bad.sum())
    v = v[~bad]
    hist[0] += int((v == 0).sum())
    v = v[v != 0]
    e = np.frexp(v)[1] - 1 + int(exp)                   # v * 2^exp in [2^e, 2^(e+1))
    for b in range(1, L.RANGE_BINS):
        lo = L.RANGE_BINADE[b]
        hi = L.RANGE_BINADE[b + 1] if b + 1 < L.RANGE_BINS else float("inf")
        hist[b] += int(((e >= lo) & (e < hi)).sum())
    return hist

