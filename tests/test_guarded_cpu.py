"""The canary harness (tests/guarded.py) can fail, shown on CPU buffers with plain torch writes; and every `dfd_*`
function of include/dfdclip.h is either in the coverage table of tests/test_hip_guarded.py or exempt here with a reason."""
import ast
import os
import re

import pytest
import torch

from tests import guarded as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dfd_* functions that need no guarded run: they touch no device memory
EXEMPT = {
    "dfd_last_error": "returns a host string",
    "dfd_abi_version": "returns a constant",
    "dfd_device_check": "queries the device, no buffers",
    "dfd_preprocess_geometry": "host-only arithmetic on host pointers",
    "dfd_gemm_last_path": "reads a thread-local host flag",
    "dfd_gemm_set_variant": "sets a thread-local host flag",
    "dfd_sgd_blocks": "host-only arithmetic",
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float8_e4m3fn])
@pytest.mark.parametrize("rows,cols,ld", [(3, 8, 12), (5, 4, 4), (1, 16, 24)])
def test_layout_and_poison(dtype, rows, cols, ld):
    g = G.guarded(rows, cols, dtype, ld=ld, device="cpu")
    esz = g.esz
    assert g.t.shape == (rows, cols) and g.t.stride() == (ld, 1) and g.t.data_ptr() % 16 == 0
    assert g.front >= 4096 and g.front % 256 == 0 and g.back % 256 == 0
    assert g.back >= min(256 * ld * esz, 8 << 20)
    assert g.flat.numel() >= g.front + rows * ld * esz + g.back
    assert torch.isnan(g.t.float()).all(), "the interior of an output starts poisoned"
    pat = G.nan_pattern(esz).to_bytes(esz, "little")
    assert bytes(g.flat[:esz].tolist()) == pat and bytes(g.flat[g.front + g.body:g.front + g.body + esz].tolist()) == pat
    g.assert_untouched()
    g.t.zero_()  # writing the view is what an output is for
    g.assert_untouched()


def test_back_guard_is_capped_at_8_mib():
    g = G.guarded(1, 8, torch.float32, ld=16384, device="cpu")
    assert g.back == 8 << 20


def _flat_elems(g):
    return g.flat[:g.flat.numel() // g.esz * g.esz].view(g.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_write_one_element_before_the_view_is_reported(dtype):
    g = G.guarded(4, 8, dtype, ld=12, device="cpu", name="y")
    g.set(torch.zeros(4, 8))
    _flat_elems(g)[g.front // g.esz - 1] = 1.0
    with pytest.raises(AssertionError, match=r"\(row -1, column 11\) \[front guard\]"):
        g.assert_untouched()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_write_one_element_after_the_view_is_reported(dtype):
    # dense rows: the element after view[rows-1, cols-1] is the first of the back guard
    g = G.guarded(4, 8, dtype, device="cpu")
    _flat_elems(g)[g.front // g.esz + 4 * 8] = 1.0
    with pytest.raises(AssertionError, match=r"\(row 4, column 0\) \[back guard\]"):
        g.assert_untouched()
    # padded rows: it is the first padding element of the last row
    g = G.guarded(4, 8, dtype, ld=12, device="cpu")
    _flat_elems(g)[g.front // g.esz + 3 * 12 + 8] = 1.0
    with pytest.raises(AssertionError, match=r"\(row 3, column 8\) \[row padding\]"):
        g.assert_untouched()
    # and behind the last row's padding the back guard starts
    g = G.guarded(4, 8, dtype, ld=12, device="cpu")
    _flat_elems(g)[g.front // g.esz + 4 * 12] = 1.0
    with pytest.raises(AssertionError, match=r"\(row 4, column 0\) \[back guard\]"):
        g.assert_untouched()


def test_write_into_row_padding_is_reported():
    g = G.guarded(5, 8, torch.float32, ld=12, device="cpu")
    g.set(torch.ones(5, 8))
    wide = g.flat[g.front:g.front + g.body].view(torch.float32).view(5, 12)
    wide[2, 9] = 3.0
    wide[4, 11] = 3.0
    with pytest.raises(AssertionError, match=r"8 byte\(s\).*\(row 2, column 9\) \[row padding\]"):
        g.assert_untouched()


def test_same_value_different_payload_is_still_a_write():
    """The comparison is on bytes: a NaN with another payload written over the poison counts."""
    g = G.guarded(2, 4, torch.float32, ld=8, device="cpu")
    wide = g.flat[g.front:g.front + g.body].view(torch.float32).view(2, 8)
    wide[0, 5] = float("nan")  # the default quiet NaN 0x7fc00000, not the poison pattern
    with pytest.raises(AssertionError, match=r"\(row 0, column 5\)"):
        g.assert_untouched()


def test_read_of_padding_yields_nan():
    g = G.guarded(3, 8, torch.float32, ld=12, device="cpu")
    g.set(torch.ones(3, 8))
    wide = g.flat[g.front:g.front + g.body].view(torch.float32).view(3, 12)
    assert torch.isfinite(g.t.sum()) and torch.isnan(wide[:, :9].sum()), "a row read one element too far is poisoned"
    assert torch.isnan(wide[:, 8:]).all()
    b = G.guarded(3, 8, torch.bfloat16, ld=16, device="cpu")
    assert torch.isnan(b.flat[b.front:b.front + b.body].view(torch.bfloat16).float()).all()
    f8 = G.guarded(3, 16, torch.float8_e4m3fn, ld=32, device="cpu")
    assert torch.isnan(f8.flat.view(torch.float8_e4m3fn).float()).all()


def test_inputs_can_be_checked_whole_and_integer_fills():
    m = G.guarded_1d(6, torch.uint8, fill=1, device="cpu")
    m.set(torch.zeros(6, dtype=torch.uint8))
    assert int(m.flat[m.front - 1]) == 1 and int(m.flat[m.front + 6]) == 1 and int(m.t.sum()) == 0
    m.assert_untouched(view_too=True)
    m.t[0, 2] = 1
    m.assert_untouched()
    with pytest.raises(AssertionError, match=r"\(row 0, column 2\) \[input view\]"):
        m.assert_untouched(view_too=True)
    with pytest.raises(AssertionError):
        G.guarded_1d(6, torch.uint8, device="cpu")  # integers need a fill


def test_exact_size_workspace():
    w = G.guarded_bytes(1000, device="cpu")
    assert w.t.shape == (1, 1000) and w.front % 256 == 0 and w.t.data_ptr() % 16 == 0
    assert torch.isnan(w.t.view(torch.float32)).all(), "an uninitialised workspace reads as NaN"
    w.t.zero_()
    w.assert_untouched()
    w.flat[w.front + 1000] = 0  # the byte directly behind the workspace
    with pytest.raises(AssertionError, match=r"\(row 1, column 0\) \[back guard\]"):
        w.assert_untouched()
    w = G.guarded_bytes(1000, device="cpu")
    w.flat[w.front - 1] = 0
    with pytest.raises(AssertionError, match=r"\[front guard\]"):
        w.assert_untouched()


# ---- every dfd_* function of the header is covered or exempt ---------------------------------------------------

def _header_functions():
    text = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", text)))


def _coverage_table():
    src = open(os.path.join(ROOT, "tests", "test_hip_guarded.py")).read()
    tree = ast.parse(src)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    table = {}
    for line in ast.get_docstring(tree).splitlines():
        m = re.match(r"\s*(dfd_[a-z0-9_]+)\s+(test_[a-z0-9_, ]+)$", line)
        if m:
            table[m.group(1)] = [t.strip() for t in m.group(2).split(",") if t.strip()]
    return table, tests, src


def test_header_parse_finds_the_abi():
    fns = _header_functions()
    assert {"dfd_gemm", "dfd_gemm_fp8", "dfd_layernorm", "dfd_sgd_step", "dfd_last_error", "dfd_gelu_erf_bwd"} <= set(fns)
    assert "dfd_dropout_t" not in fns and "dfd_gemm_extra" not in fns and len(fns) >= 45


def test_every_abi_function_is_in_the_guarded_table_or_exempt():
    table, tests, src = _coverage_table()
    fns = _header_functions()
    missing = [f for f in fns if f not in table and f not in EXEMPT]
    assert not missing, f"new ABI functions without a guarded test or an exemption: {missing}"
    both = [f for f in fns if f in table and f in EXEMPT]
    assert not both, f"listed and exempt at once: {both}"
    stale = [f for f in list(table) + list(EXEMPT) if f not in fns]
    assert not stale, f"not in the header any more: {stale}"
    for f, ts in table.items():
        assert ts, f
        for t in ts:
            assert t in tests, f"{f}: the table names {t}, which tests/test_hip_guarded.py does not define"
        # the covering test really calls it: through capi.<name without dfd_> or its *_bytes wrapper
        stem = f[len("dfd_"):]
        names = {stem, stem + "_bytes", stem.replace("_f32", "")}
        assert any(re.search(r"\bcapi\.%s\(" % re.escape(n), src) for n in names), f"{f}: no call through capi in the module"
    assert all(len(r) > 8 for r in EXEMPT.values())
