"""Encoder attention at any token count, through `capi.attention_fwd` on the guarded harness of tests/test_hip_guarded.py
(ld_qkv = 3D + 8, ld_out = D + 8, NaN guards and row padding, NaN-filled outputs, dense = guarded bit for bit).

* bf16, 33 tokens and up outside the 193..224 / 257..288 windows: the streaming MFMA kernel (attention_mfma_any.hip).
  It walks the keys in chunks of 128 and gives a workgroup a span of 128 queries, so the counts sit on both sides of every
  chunk, span and 32-row block edge: 33, 64 | 65, 127 | 128 | 129, 160, 192, 225, 226, 256, 289, 577, 640 | 641, 1370.
* Where the running maximum lands (577 tokens = 4 full chunks + 65 keys): first chunk, last chunk, rising with the key
  index (every chunk rescales), and a common score offset large enough that exp2 overflows (or everything underflows)
  unless the maximum is subtracted first.
* f32 and the bf16 fallback: the rows kernel with K and V staged in key chunks — bit-identical to the whole-head staging
  where both run (variant 1 against 0), and the only form above 160 KiB of K and V (f32 above 320 tokens).

Reference: softmax in fp64 on the same rounded operands.  Bars: the project's existing ones for this entry point,
(2e-2, 2^-7) for bf16 and (2e-5, 1e-5) for f32 (test_attention_fwd)."""
import functools

import pytest
import torch

from tests.test_hip_guarded import BF16, F32, both, rnd, same_bits, verify

pytestmark = pytest.mark.gpu

BF16_TOL = (2e-2, 2 ** -7)
F32_TOL = (2e-5, 1e-5)
CHUNK = 128  # keys per chunk of the streaming kernel


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    yield c
    c.attention_set_variant(0)


def scores64(qkv, n, tokens, heads):
    """fp64 q·kᵀ/8 [n, heads, q, k] and v [n, heads, k, 64] of a packed (already rounded) projection, on the GPU."""
    t = qkv.cuda().double().view(n, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0] @ t[1].transpose(-1, -2) / 8.0, t[2]


def reference(qkv, n, tokens, heads):
    s, v = scores64(qkv, n, tokens, heads)
    return (s.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(n * tokens, heads * 64).cpu()


@functools.lru_cache(maxsize=None)
def random_case(n, tokens, heads, dtype):
    D = heads * 64
    qkv = rnd(n * tokens, 3 * D, seed=16 + tokens)
    qkv[:, :D] *= 2.0
    qkv = qkv.to(dtype)
    return qkv, reference(qkv, n, tokens, heads)


def run(capi, qkv, n, tokens, heads, want, tol, msg, path, variant=0):
    """`path`: the kernel (capi.ATTN_*) that both the dense and the guarded call (ld + 8) must take."""
    D = heads * 64

    def op(b):
        out = b.out((n * tokens, D), qkv.dtype, pad=8, name="out")
        capi.attention_fwd(b.inp(qkv, pad=8, name="qkv"), out, n, tokens, heads)
        assert capi.attention_last_path() == path, f"{msg}: {'guarded' if b.guard else 'dense'} call took kernel {capi.attention_last_path()}, not {path}"
        return {"out": out}
    capi.attention_set_variant(variant)
    try:
        dense, got = both(op)
    finally:
        capi.attention_set_variant(0)
    verify(dense, got, {"out": (want, *tol)}, msg=msg)
    return dense["out"]


TOKENS = [33, 50, 64, 65, 127, 128, 129, 160, 192, 225, 226, 256, 289, 577, 640, 641, 1370]
BF16_CASES = [(n, t, h) for t in TOKENS for h in (2, 12) for n in ((1,) if t == 1370 else (1, 3))]


@pytest.mark.parametrize("n,tokens,heads", BF16_CASES)
def test_bf16_streaming_kernel(capi, n, tokens, heads):
    qkv, want = random_case(n, tokens, heads, BF16)
    run(capi, qkv, n, tokens, heads, want, BF16_TOL, f"bf16 {n}x{tokens}x{heads}", capi.ATTN_STREAM)


# ---- where the running maximum lands ------------------------------------------------------------------------------

def max_case(kind):
    """[577, 3*128] bf16 (1 frame, 2 heads).  Channel 0 of q is 8 (1 after the scale) against a designed k channel 0;
    `offset±`: channel 1 of q is ±60 against k channel 1 = 16, a common raw offset of ±960 = ±173 in the exponent of 2."""
    tokens, heads, D = 577, 2, 128
    qkv = rnd(tokens, 3 * D, seed=77)
    qkv[:, :D] *= 0.5          # the random part of a score: sigma ~ 0.5
    key = torch.arange(tokens, dtype=torch.float32)
    for h in range(heads):
        q0, k0 = h * 64, D + h * 64
        if kind in ("first", "last", "rising"):
            qkv[:, q0] = 8.0
            qkv[:, k0] = {"first": 8.0 * (key == 3), "last": 8.0 * (key == tokens - 1), "rising": key / 8.0}[kind]
        else:
            qkv[:, q0 + 1] = 60.0 if kind == "offset+" else -60.0
            qkv[:, k0 + 1] = 16.0
    return qkv.to(BF16), tokens, heads


@pytest.mark.parametrize("kind", ["first", "last", "rising", "offset+", "offset-"])
def test_bf16_running_maximum(capi, kind):
    qkv, tokens, heads = max_case(kind)
    s, v = scores64(qkv, 1, tokens, heads)
    want = reference(qkv, 1, tokens, heads)
    assert torch.isfinite(want).all(), "the fp64 reference itself must be finite"
    # the case is what it claims to be
    nch = (tokens + CHUNK - 1) // CHUNK
    cmax = torch.stack([s[..., c * CHUNK:(c + 1) * CHUNK].amax(dim=-1) for c in range(nch)], dim=-1)  # [1, h, q, chunk]
    if kind == "first":
        assert (cmax.argmax(dim=-1) == 0).all()
    elif kind == "last":
        assert (cmax.argmax(dim=-1) == nch - 1).all() and tokens % CHUNK != 0
    elif kind == "rising":
        assert (cmax[..., 1:] > cmax[..., :-1]).all(), "every chunk raises the maximum of every query"
    else:
        e2 = s * 1.4426950408889634
        assert (e2.amax(dim=-1) > 128).all() if kind == "offset+" else (e2.amax(dim=-1) < -150).all()
    # a kernel that rounds P to bf16 for the second product stays inside the bar: the bar is fair for this case
    p = (s - s.amax(dim=-1, keepdim=True)).exp()
    emu = (p.to(BF16).double() @ v / p.sum(dim=-1, keepdim=True)).permute(0, 2, 1, 3).reshape(tokens, heads * 64).cpu()
    assert ((emu - want).abs() <= BF16_TOL[0] + BF16_TOL[1] * want.abs()).all()
    run(capi, qkv, 1, tokens, heads, want, BF16_TOL, f"bf16 max {kind}", capi.ATTN_STREAM)


# ---- launch independence ------------------------------------------------------------------------------------------

def test_bf16_whole_launch_equals_chunks_of_three_frames(capi):
    n, tokens, heads = 40, 577, 16
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(n * tokens, 3 * D, device="cuda", generator=g).to(BF16)
    whole = torch.empty(n * tokens, D, device="cuda", dtype=BF16)
    capi.attention_fwd(qkv, whole, n, tokens, heads)
    parts = torch.empty_like(whole)
    for f0 in range(0, n, 3):
        k = min(3, n - f0)
        capi.attention_fwd(qkv[f0 * tokens:(f0 + k) * tokens], parts[f0 * tokens:(f0 + k) * tokens], k, tokens, heads)
    torch.cuda.synchronize()
    assert torch.isfinite(whole.float()).all()
    same_bits(whole, parts, "40 frames at once and in chunks of 3")


# ---- the rows kernel with chunked staging -------------------------------------------------------------------------

@pytest.mark.parametrize("tokens", [64, 197, 320])
def test_f32_chunked_staging_is_bit_identical(capi, tokens):
    n, heads = 3, 2
    qkv, want = random_case(n, tokens, heads, F32)
    whole = run(capi, qkv, n, tokens, heads, want, F32_TOL, f"f32 {tokens} whole-head", capi.ATTN_ROWS)
    chunked = run(capi, qkv, n, tokens, heads, want, F32_TOL, f"f32 {tokens} 16-key chunks", capi.ATTN_ROWS_CHUNKED, variant=1)
    same_bits(whole, chunked, f"f32 {tokens}: chunked and whole-head staging")


@pytest.mark.parametrize("n,tokens", [(2, 321), (2, 577), (1, 1370)])
def test_f32_above_the_lds_ceiling(capi, n, tokens):
    heads = 2
    qkv, want = random_case(n, tokens, heads, F32)
    run(capi, qkv, n, tokens, heads, want, F32_TOL, f"f32 {n}x{tokens}", capi.ATTN_ROWS_CHUNKED)


def test_bf16_fallback_above_the_lds_ceiling(capi):
    """641 tokens with the streaming kernel skipped: 164,096 B of K and V, the rows kernel's chunked form."""
    n, tokens, heads = 2, 641, 2
    qkv, want = random_case(n, tokens, heads, BF16)
    run(capi, qkv, n, tokens, heads, want, BF16_TOL, "bf16 641 rows kernel", capi.ATTN_ROWS_CHUNKED, variant=2)
