"""`dfd_ema_step` (include/dfdclip_ema.h, csrc/optim.hip) on the GPU: every teacher tensor and every transposed copy equals the
torch expression `(1 - r) * t + r * s` evaluated on the same device, bit for bit (`torch.equal`; a mirror equals the transposed
new parameter), over flat and mirrored entries at the block and tile edges, tables of 1, 2, 3 and 40 mixed entries (the binary
search over `first_block`), both stream-policy settings, with guard bands (tests/guarded.py) round every teacher tensor and
mirror untouched and the student tensors unchanged; and the refusals raise before anything is launched."""
import pytest
import torch

from tests.guarded import guarded_1d

pytestmark = pytest.mark.gpu

FLATS = [1, 255, 256, 1023, 1024, 1025, 3 * 1024 + 1]
MIRRORS = [(1, 1), (1, 40), (40, 1), (31, 33), (32, 32), (33, 65), (64, 96)]
RATIOS = [0.0, 0.5, 0.999, 1.0]


def mixed(n):
    """n entries, flat and mirrored in turn, cycling through every size above."""
    out = []
    for i in range(n):
        out.append(MIRRORS[(i // 2) % len(MIRRORS)] if i % 2 else FLATS[(i // 2) % len(FLATS)])
    return out


TABLES = {"flats": FLATS, "mirrors": MIRRORS, "one_flat": [1025], "one_mirror": [(33, 65)], "two": mixed(2), "three": mixed(3),
          "forty": mixed(40)}


class Entry:
    def __init__(self, spec, seed, special=False):
        g = torch.Generator().manual_seed(seed)
        self.shape = spec if isinstance(spec, tuple) else (spec,)
        n = 1
        for d in self.shape:
            n *= d
        t0, s0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 2.5
        if special and n >= 8:
            tiny = 1.401298464324817e-45
            t0[:8] = torch.tensor([0.0, -0.0, tiny, -tiny, 1.1e-38, -5.9e-39, 3.0e38, -3.0e38])
            s0[:8] = torch.tensor([-0.0, 0.0, -tiny, 5.9e-39, tiny, 1.1e-38, 3.0e38, 3.0e38])
        self.t0 = t0.cuda()
        self.t = guarded_1d(n, torch.float32, name=f"teacher{seed}").set(t0)
        self.s = guarded_1d(n, torch.float32, name=f"student{seed}").set(s0)
        self.m = guarded_1d(n, torch.float32, name=f"mirror{seed}") if len(self.shape) == 2 else None
        self.numel = n

    def row(self, capi, first):
        rows, cols = self.shape if self.m is not None else (0, 0)
        r = [self.t.t.data_ptr(), self.s.t.data_ptr(), 0, 0 if self.m is None else self.m.t.data_ptr(), self.numel, rows | (cols << 32), first]
        return r, capi.sgd_blocks(self.numel, rows, cols, self.m is not None)

    def reset(self):
        self.t.t.copy_(self.t0.view(1, -1))


def build_table(capi, entries):
    rows, first = [], 0
    for e in entries:
        r, blocks = e.row(capi, first)
        rows.append(r)
        first += blocks
    host = torch.tensor(rows, dtype=torch.int64)
    return host, host.cuda(), first


def check(capi, entries, r, what):
    host, table, blocks = build_table(capi, entries)
    was = capi.stream_policy_get()
    results = []
    try:
        for mask in (was | capi.STREAM_OPTIMIZER, was & ~capi.STREAM_OPTIMIZER):
            capi.stream_policy_set(mask)
            for e in entries:
                e.reset()
            capi.ema_step(table, len(entries), blocks, r, table_host=host)
            torch.cuda.synchronize()
            got = []
            for i, e in enumerate(entries):
                want = (1 - r) * e.t0 + r * e.s.t.view(-1)  # the reference's expression, on this device
                new = e.t.t.view(-1)
                assert torch.equal(new, want), f"{what}: entry {i} {e.shape} at r={r}, policy {mask}: {(new != want).sum().item()} elements differ"
                assert torch.equal(new, capi.ema_reference(e.t0, e.s.t.view(-1), r))
                e.t.assert_untouched()
                e.s.assert_untouched(view_too=True)
                if e.m is not None:
                    assert torch.equal(e.m.t.view(e.shape[1], e.shape[0]), new.view(e.shape).t()), f"{what}: mirror of entry {i} {e.shape}"
                    e.m.assert_untouched()
                got.append(new.clone())
            results.append(got)
    finally:
        capi.stream_policy_set(was)
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: the two stream policies differ"


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi
    capi.load_library()
    return capi


@pytest.mark.parametrize("r", RATIOS)
@pytest.mark.parametrize("name", list(TABLES))
def test_ema_step_equals_the_torch_expression(capi, name, r):
    entries = [Entry(spec, 100 * i + len(TABLES[name])) for i, spec in enumerate(TABLES[name])]
    check(capi, entries, r, name)


@pytest.mark.parametrize("r", [0.3, 0.95, 0.999])
def test_signed_zeros_denormals_and_large_values(capi, r):
    entries = [Entry(spec, 7 + i, special=True) for i, spec in enumerate([1025, (33, 65), 255, (4, 2)])]
    check(capi, entries, r, "special values")


def test_non_finite_elements_follow_ieee(capi):
    e = Entry(8, 1)
    t0 = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0, float("inf"), 0.0, 2.0, -1.0])
    s0 = torch.tensor([float("inf"), float("inf"), 1.0, float("nan"), 0.0, float("inf"), float("-inf"), -1.0])
    e.t0 = t0.cuda()
    e.s.set(s0)
    for r in (0.0, 0.5, 1.0):
        e.reset()
        host, table, blocks = build_table(capi, [e])
        capi.ema_step(table, 1, blocks, r, table_host=host)
        want = (1 - r) * e.t0 + r * e.s.t.view(-1)
        got = e.t.t.view(-1)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan]), (r, got, want)
        e.t.assert_untouched()


def test_refusals_raise_before_any_launch(capi):
    entries = [Entry(1025, 1), Entry((33, 65), 2)]
    host, table, blocks = build_table(capi, entries)

    def refused(match, tab_host, *args, **kw):
        with pytest.raises(capi.DfdError, match=match):
            capi.ema_step(*args, table_host=tab_host, **kw)
        torch.cuda.synchronize()
        for e in entries:
            assert torch.equal(e.t.t.view(-1), e.t0), "a refused call wrote the teacher"
            e.t.assert_untouched()

    alias = host.clone()
    alias[1, 1] = alias[1, 0]
    refused("p == g", alias, alias.cuda(), 2, blocks, 0.5)
    refused("p == g", None, alias.cuda(), 2, blocks, 0.5)  # (without the host copy the table is read back)
    buf = host.clone()
    buf[0, 2] = entries[0].s.t.data_ptr()
    refused("buf must be NULL", buf, buf.cuda(), 2, blocks, 0.5)
    refused("empty table", host[:0], table[:0], 0, blocks, 0.5)
    refused("total_blocks", host, table, 2, 0, 0.5)
    refused("total_blocks", host, table, 2, 1 << 31, 0.5)
    refused("non-finite", host, table, 2, blocks, float("nan"))
    refused("non-finite", host, table, 2, blocks, float("inf"))
    capi.ema_step(table, 2, blocks, 0.5, table_host=host)  # and the same table goes through
    assert torch.equal(entries[0].t.t.view(-1), 0.5 * entries[0].t0 + 0.5 * entries[0].s.t.view(-1))
