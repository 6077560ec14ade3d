"""Canary buffers for the C-ABI tests: a tensor view inside one flat allocation the test owns, with poisoned guards in
front of and behind it and poisoned padding between its rows.

    flat = [ front guard | row 0 . pad | row 1 . pad | ... | row rows-1 . pad | back guard ]

* front guard >= 4 KiB; back guard >= 256 rows of `ld` elements (one tile of rows), 8 MiB where that would be more;
  both are multiples of 256 B, so the view keeps the alignment of the allocation (16 B and better).
* Guards, padding and the interior of the view start as a NaN with a recognisable payload (f32 0x7fc5a5a5, bf16
  0x7fc5, one-byte floats 0x7f = the e4m3 NaN).  A load from there poisons the result; an element that is never
  written stays NaN.  Integer buffers take `fill=` (255 for uint8 pixels, 1 for frame-mask bytes: values that change
  the result when they are read).
* `assert_untouched()` compares every byte outside the view with a snapshot taken after the last `set()` — on a uint8
  view, so NaN payloads count — and reports the first offending byte as (row, column) relative to the view:
  row = floor(e / ld), column = e mod ld for the element offset e from view[0, 0] (negative rows: front guard; columns
  >= cols: row padding; rows >= rows: back guard).

Plain torch, any device: tests/test_guarded_cpu.py proves on CPU buffers that the harness can fail.
"""
import torch

FRONT_MIN = 4096
BACK_ROWS = 256
BACK_MAX = 8 << 20
GRAIN = 256

# element size -> (torch dtype to fill through, NaN bit pattern)
_NAN = {4: (torch.int32, 0x7FC5A5A5), 2: (torch.int16, 0x7FC5), 1: (torch.uint8, 0x7F)}


def _round_up(n, m):
    return (n + m - 1) // m * m


def nan_pattern(esz):
    """The poison value of an `esz`-byte float, as an integer."""
    return _NAN[esz][1]


class Guarded:
    """One guarded buffer.  `.t` is the [rows, cols] view (row stride `ld`); `.flat` the uint8 allocation."""

    def __init__(self, rows, cols, dtype, ld=None, fill=None, device="cuda", front=None, back=None, name=""):
        ld = cols if ld is None else int(ld)
        assert rows >= 0 and cols > 0 and ld >= cols, (rows, cols, ld)
        esz = torch.empty(0, dtype=dtype).element_size()
        self.rows, self.cols, self.ld, self.esz, self.dtype, self.name = rows, cols, ld, esz, dtype, name
        self.front = _round_up(FRONT_MIN, GRAIN) if front is None else front
        self.body = rows * ld * esz
        if back is None:
            back = _round_up(max(min(BACK_ROWS * ld * esz, BACK_MAX), GRAIN), GRAIN)
        self.back = back
        assert self.front % GRAIN == 0 and self.back % GRAIN == 0 and self.front >= FRONT_MIN
        total = _round_up(self.front + self.body + self.back, 4)
        self.flat = torch.empty(total, dtype=torch.uint8, device=device)
        if fill is None:
            assert dtype.is_floating_point, "integer buffers need an explicit fill"
            fdt, pat = _NAN[esz]
            if esz == 1:
                self.flat.fill_(pat)
            else:
                # two's-complement value of the pattern in the signed fill dtype
                bits = 8 * esz
                self.flat.view(fdt).fill_(pat - (1 << bits) if pat >= 1 << (bits - 1) else pat)
        else:
            assert esz == 1 and 0 <= int(fill) <= 255, "fill= is for one-byte integer buffers"
            self.flat.fill_(int(fill))
        body = self.flat[self.front:self.front + self.body].view(dtype)
        self.t = body.view(rows, ld)[:, :cols] if rows > 0 else body.view(0, ld)[:, :cols]
        assert self.t.data_ptr() % 16 == 0, "the ABI wants 16-byte aligned buffers"
        self._snap = self.flat.clone()

    # ---- contents -------------------------------------------------------------------------------------------
    def set(self, data):
        """Copy `data` (anything that reshapes to [rows, cols]) into the view; returns self."""
        self.t.copy_(data.reshape(self.rows, self.cols).to(self.t.device))
        self._snap = self.flat.clone()
        return self

    def shaped(self, *shape):
        """The view under another shape (contiguous buffers only: ld == cols)."""
        assert self.ld == self.cols, "only a dense guarded buffer can be reshaped"
        return self.flat[self.front:self.front + self.body].view(self.dtype).view(*shape)

    # ---- the check ------------------------------------------------------------------------------------------
    def _coords(self, byte_off):
        e = (byte_off - self.front) // self.esz  # floor: negative in the front guard
        return e // self.ld, e % self.ld

    def assert_untouched(self, view_too=False):
        """Every byte outside the view equals the snapshot (`view_too`: the view as well — an input)."""
        if self.flat.is_cuda:
            torch.cuda.synchronize()
        diff = self.flat != self._snap
        if not view_too and self.rows > 0:
            body = diff[self.front:self.front + self.body].view(self.rows, self.ld * self.esz)
            body[:, :self.cols * self.esz] = False
        if not bool(diff.any()):
            return
        off = int(diff.nonzero()[0, 0])
        row, col = self._coords(off)
        where = ("front guard" if off < self.front else "back guard" if off >= self.front + self.body else
                 "row padding" if col >= self.cols else "input view")
        raise AssertionError(f"{self.name or 'buffer'}: {int(diff.sum())} byte(s) outside the view were written; first at byte "
                             f"{off - self.front:+d} from the view = (row {row}, column {col}) [{where}] of a "
                             f"[{self.rows}, {self.cols}] view with ld {self.ld}, {self.esz}-byte elements")


def guarded(rows, cols, dtype, ld=None, fill=None, device="cuda", name=""):
    """A [rows, cols] view with row stride `ld >= cols` between two guards (see the module docstring)."""
    return Guarded(rows, cols, dtype, ld=ld, fill=fill, device=device, name=name)


def guarded_1d(n, dtype, fill=None, device="cuda", name=""):
    """Contiguous-only variant for kernels that take no leading dimension: `.t` is [1, n], `.shaped(...)` any shape;
    the guards sit directly in front of the first and behind the last element."""
    esz = torch.empty(0, dtype=dtype).element_size()
    back = _round_up(min(max(n * esz, FRONT_MIN), BACK_MAX), GRAIN)
    return Guarded(1, n, dtype, fill=fill, device=device, back=back, name=name)


def guarded_bytes(nbytes, device="cuda", name=""):
    """Exact-size variant for workspaces: exactly `nbytes` bytes (what a `*_workspace` function returned), poisoned
    like an f32 buffer, with the guard directly behind the last byte.  `.t` is the [1, nbytes] uint8 view."""
    nbytes = int(nbytes)
    g = Guarded.__new__(Guarded)
    g.rows, g.cols, g.ld, g.esz, g.dtype, g.name = 1, max(nbytes, 1), max(nbytes, 1), 1, torch.uint8, name
    g.front = _round_up(FRONT_MIN, GRAIN)
    g.body = nbytes
    g.back = _round_up(min(max(nbytes, FRONT_MIN), BACK_MAX), GRAIN)
    total = _round_up(g.front + g.body + g.back, 4)
    g.flat = torch.empty(total, dtype=torch.uint8, device=device)
    g.flat.view(torch.int32).fill_(_NAN[4][1])  # f32 poison, in phase with the start of the workspace
    g.t = g.flat[g.front:g.front + nbytes].view(1, nbytes) if nbytes else g.flat[g.front:g.front].view(1, 0)
    g.rows = 1 if nbytes else 0
    g._snap = g.flat.clone()
    return g
