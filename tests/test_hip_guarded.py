"""Guard-band and strided-view parity of every C-ABI kernel (tests/guarded.py).

Each case runs an entry point twice: on dense tensors that own their allocation, as the rest of the suite does, and on
guarded views — leading dimension > columns wherever the ABI takes one, poisoned guards in front and behind, poisoned row
padding, outputs NaN inside, workspaces of exactly the size the `*_workspace` function reports.  Asserted every time:
(a) no byte outside a view changed (inputs: no byte at all), (b) the outputs are finite, (c) they match the
high-precision reference at the tolerance of the kernel's existing test, (d) guarded and dense results are the same bits
whenever both calls ran the same kernel family (dfd_gemm: by gemm_last_path(), 256 and 257 one family).

Coverage (checked against include/dfdclip.h by tests/test_guarded_cpu.py):

    dfd_layernorm                         test_layernorm
    dfd_layernorm2                        test_layernorm2
    dfd_add_layernorm                     test_add_layernorm
    dfd_layernorm_bwd                     test_layernorm_bwd
    dfd_gemm                              test_gemm_general_path, test_gemm_tuned_paths, test_gemm_tuned_ldw_fallback
    dfd_gemm_fp8                          test_gemm_fp8
    dfd_gemm_at_b_workspace               test_gemm_at_b
    dfd_gemm_at_b                         test_gemm_at_b
    dfd_attention_fwd                     test_attention_fwd
    dfd_linear_rows                       test_linear_rows
    dfd_linear_rows_t_workspace           test_linear_rows_t
    dfd_linear_rows_t                     test_linear_rows_t
    dfd_linear_rows_bwd_weight            test_linear_rows_bwd_weight
    dfd_transpose_f32                     test_transpose
    dfd_head_fwd                          test_head
    dfd_head_bwd                          test_head
    dfd_decoder_attn_workspace            test_decoder_attention
    dfd_decoder_attn_fwd                  test_decoder_attention
    dfd_decoder_attn_modes_fwd            test_decoder_attention
    dfd_decoder_attn_modes_bwd            test_decoder_attention
    dfd_decoder_attn_bwd_workspace        test_decoder_attention
    dfd_decoder_attn_bwd                  test_decoder_attention
    dfd_dropout                           test_dropout
    dfd_quickgelu                         test_quickgelu
    dfd_gelu_erf                          test_gelu_erf
    dfd_gelu_erf_bwd                      test_gelu_erf
    dfd_adapter_norm_gelu                 test_adapter_norm_gelu
    dfd_adapter_norm_gelu_bwd_workspace   test_adapter_norm_gelu
    dfd_adapter_norm_gelu_bwd             test_adapter_norm_gelu
    dfd_adapter_bn_workspace              test_adapter_bn
    dfd_adapter_bn_stats                  test_adapter_bn
    dfd_adapter_bn_apply                  test_adapter_bn
    dfd_adapter_bn_bwd                    test_adapter_bn
    dfd_compinv_loss_workspace            test_compinv_loss
    dfd_compinv_loss_fwd                  test_compinv_loss
    dfd_compinv_loss_bwd                  test_compinv_loss
    dfd_patchify                          test_patchify
    dfd_preprocess_u8                     test_preprocess_u8
    dfd_sgd_step                          test_sgd_step
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dropout_mask, ref_cpu
from tests.guarded import guarded, guarded_1d, guarded_bytes, nan_pattern

pytestmark = pytest.mark.gpu

F32, BF16, E4M3 = torch.float32, torch.bfloat16, torch.float8_e4m3fn
RT16 = 2.0 ** -8  # bf16 results: half an ulp is 2^-9 (tests/test_hip_kernels.py)


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


# ---- the dense / guarded buffer factory --------------------------------------------------------------------------

def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    esz = t.element_size()
    if t.numel():
        t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[esz]).fill_(
            nan_pattern(esz) - (1 << 8 * esz) if esz > 1 and nan_pattern(esz) >= 1 << (8 * esz - 1) else nan_pattern(esz))
    return t


class Bufs:
    """`guard` False: dense tensors that own their allocation.  True: the same tensors as guarded views."""

    def __init__(self, guard):
        self.guard, self.items = guard, []

    def inp(self, data, pad=0, fill=None, name="in"):
        data = data.cuda()
        if not self.guard:
            return data.contiguous()
        if data.dim() == 2:
            g = guarded(data.shape[0], data.shape[1], data.dtype, ld=data.shape[1] + pad, fill=fill, name=name).set(data)
            self.items.append((g, True))
            return g.t
        g = guarded_1d(data.numel(), data.dtype, fill=fill, name=name).set(data.reshape(1, -1))
        self.items.append((g, True))
        return g.shaped(*data.shape)

    def out(self, shape, dtype=F32, pad=0, init=None, name="out"):
        shape = tuple(shape)
        if not self.guard:
            t = _poisoned(shape, dtype)
            if init is not None:
                t.copy_(init.reshape(shape))
            return t
        if len(shape) == 2:
            g = guarded(shape[0], shape[1], dtype, ld=shape[1] + pad, name=name)
            t = g.t
        else:
            g = guarded_1d(math.prod(shape), dtype, name=name)
            t = g.shaped(*shape)
        if init is not None:
            g.set(init)
        self.items.append((g, False))
        return t

    def ws(self, nbytes, name="workspace"):
        """A workspace of exactly `nbytes` bytes, contents poisoned (a kernel may not assume zeros)."""
        if not self.guard:
            return _poisoned(((int(nbytes) + 3) // 4 * 4,), torch.uint8)
        g = guarded_bytes(nbytes, name=name)
        self.items.append((g, False))
        return g.t.view(-1)

    def check(self):
        torch.cuda.synchronize()
        for g, is_input in self.items:
            g.assert_untouched(view_too=is_input)


def both(op):
    """Run `op(bufs) -> {name: output}` dense, then guarded; (a) is asserted here."""
    dense = op(Bufs(False))
    torch.cuda.synchronize()
    b = Bufs(True)
    got = op(b)
    b.check()
    return dense, got


def _f(t):
    return t.view(E4M3).double() if t.element_size() == 1 else t.double()


def close(got, want, atol, rtol=0.0, msg=""):
    got, want = _f(got.detach()).cpu(), want.detach().double().cpu().reshape(got.shape)
    assert torch.isfinite(got).all(), f"{msg}: non-finite output (poison was read, or an element was never written)"
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    bad = err > lim
    assert not bad.any(), f"{msg}: max err {err.max().item():.3e} at {tuple(bad.nonzero()[0].tolist())}, {int(bad.sum())} elements over"


def same_bits(a, b, msg=""):
    ia = a.contiguous().view(torch.uint8)
    ib = b.contiguous().view(torch.uint8)
    assert a.shape == b.shape and torch.equal(ia, ib), f"{msg}: guarded and dense results differ in their bits"


def verify(dense, got, refs, same=True, msg=""):
    """(b), (c) on both runs and (d); refs: name -> (reference, atol, rtol)."""
    for name, (ref, atol, rtol) in refs.items():
        close(got[name], ref, atol, rtol, f"{msg} {name} (guarded)")
        close(dense[name], ref, atol, rtol, f"{msg} {name} (dense)")
    for name in got:
        if name not in refs:
            assert torch.isfinite(_f(got[name])).all(), f"{msg} {name}: non-finite"
        if same:
            same_bits(dense[name], got[name], f"{msg} {name}")


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


# ---- LayerNorm family ---------------------------------------------------------------------------------------------

LN_ROWS = [1, 3, 5, 1001]
LN_COLS = [4, 132, 260, 772, 1024, 2048]
FP8_SCALE = 0.02


def _ln_tol(dtype):
    return (2e-5, 0.0) if dtype == F32 else (1e-5, RT16)


def _check_ln_out(d, g, name, want, dtype, msg):
    """f32 / bf16: the tolerances of test_layernorm.  e4m3: test_fp8_layernorm_output's bound — every element within one
    e4m3 step (2^-3 relative + half a subnormal) of the rounded reference, and at most 2e-3 of them (the two LayerNorms
    differ in the last f32 bits, so a result on a rounding boundary may fall either way) — at least 2 elements, since
    2e-3 of a 4-element row is none — off at all."""
    if dtype != E4M3:
        verify(d, g, {name: (want, *_ln_tol(dtype))}, msg=msg)
        return
    ref8 = (want / FP8_SCALE).clamp(-448, 448).float().to(E4M3).double()
    for run in (d, g):
        got = _f(run[name]).cpu()
        assert torch.isfinite(got).all(), f"{msg}: non-finite e4m3 output"
        mism = got != ref8.cpu()
        assert ((got - ref8.cpu()).abs() <= 2 ** -3 * ref8.cpu().abs() + 2 ** -9).all(), msg
        assert int(mism.sum()) <= max(2, 2e-3 * mism.numel()), msg
    same_bits(d[name], g[name], msg)


def _ln_inputs(rows, cols):
    x = rnd(rows, cols, seed=rows + cols, scale=3.0) + 0.5
    gam, bet = 1 + 0.1 * rnd(cols, seed=2), 0.1 * rnd(cols, seed=3)
    return x, gam, bet


@pytest.mark.parametrize("cols", LN_COLS + [3072, 4096])
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm(capi, rows, cols):
    x, gam, bet = _ln_inputs(rows, cols)
    want = F.layer_norm(x.double(), (cols,), gam.double(), bet.double(), 1e-5)
    for dtype in (F32, BF16, E4M3):
        def op(b):
            y = b.out((rows, cols), dtype, pad=8, name="y")
            capi.layernorm(b.inp(x, pad=4, name="x"), b.inp(gam, name="gamma"), b.inp(bet, name="beta"), y,
                           out_inv_scale=1.0 / FP8_SCALE if dtype == E4M3 else 0.0)
            return {"y": y}
        d, g = both(op)
        _check_ln_out(d, g, "y", want, dtype, f"layernorm {dtype}")

    def op(b):  # in place (f32)
        xx = b.out((rows, cols), F32, pad=4, init=x, name="x")
        capi.layernorm(xx, b.inp(gam), b.inp(bet), xx)
        return {"x": xx}
    verify(*both(op), {"x": (want, 2e-5, 0.0)}, msg="layernorm in place")


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm2(capi, rows, cols):
    x, ga, ba = _ln_inputs(rows, cols)
    gb, bb = 1 + 0.5 * rnd(cols, seed=5), 0.5 * rnd(cols, seed=6)
    xa = F.layer_norm(x.double(), (cols,), ga.double(), ba.double(), 1e-5)
    # the second LayerNorm is taken of the f32-rounded first one, as the kernel stores and re-reads it
    want = F.layer_norm(xa.float().double(), (cols,), gb.double(), bb.double(), 1e-5)
    for dtype in (F32, BF16, E4M3):
        def op(b):
            xx = b.out((rows, cols), F32, pad=4, init=x, name="x")
            y = b.out((rows, cols), dtype, pad=12, name="y")
            capi.layernorm2(xx, b.inp(ga), b.inp(ba), b.inp(gb), b.inp(bb), y, out_inv_scale=1.0 / FP8_SCALE if dtype == E4M3 else 0.0)
            return {"x": xx, "y": y}
        d, g = both(op)
        verify(d, g, {"x": (xa, 2e-5, 0.0)}, msg=f"layernorm2 {dtype}")
        # 2e-5 on x moves LayerNorm_b(x) by up to |gamma_b| * 2e-5 / std(x) ~ 1e-4: compare y with the kernel's own x
        for run in (d, g):
            wy = F.layer_norm(run["x"].double().cpu(), (cols,), gb.double(), bb.double(), 1e-5)
            _check_ln_out({"y": run["y"]}, {"y": run["y"]}, "y", wy, dtype, f"layernorm2 y {dtype}")
    assert want.shape == (rows, cols)


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("delta_dtype", [F32, BF16])
def test_add_layernorm(capi, rows, cols, delta_dtype):
    x, gam, bet = _ln_inputs(rows, cols)
    d1, d2 = rnd(rows, cols, seed=4).to(delta_dtype), rnd(rows, cols, seed=5).to(delta_dtype)
    for two in (False, True):
        v = x + d1.float() if not two else (x + d1.float()) + d2.float()
        want = F.layer_norm(v.double(), (cols,), gam.double(), bet.double(), 1e-5)
        for dtype in (F32, BF16, E4M3):
            for store_x in (True, False):
                def op(b):
                    xx = b.out((rows, cols), F32, pad=4, init=x, name="x")
                    y = b.out((rows, cols), dtype, pad=8, name="y")
                    capi.add_layernorm(xx, b.inp(d1, pad=12, name="delta"), b.inp(gam), b.inp(bet), y,
                                       delta2=b.inp(d2, pad=12, name="delta2") if two else None, store_x=store_x,
                                       out_inv_scale=1.0 / FP8_SCALE if dtype == E4M3 else 0.0)
                    return {"x": xx, "y": y}
                d, g = both(op)
                msg = f"add_layernorm two={two} {dtype} store_x={store_x}"
                for run in (d, g):
                    assert torch.equal(run["x"].cpu(), v if store_x else x), f"{msg}: x must hold the exact fp32 sum / stay untouched"
                _check_ln_out(d, g, "y", want, dtype, msg)


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_bwd(capi, rows, cols):
    x = (rnd(rows, cols, seed=8, scale=2.0) + 0.3).double().requires_grad_(True)
    gam = (1 + 0.1 * rnd(cols, seed=9)).double().requires_grad_(True)
    bet = (0.1 * rnd(cols, seed=10)).double().requires_grad_(True)
    dy, dx0 = rnd(rows, cols, seed=11), rnd(rows, cols, seed=12)
    (F.layer_norm(x, (cols,), gam, bet, 1e-5) * dy.double()).sum().backward()
    for acc in (False, True):
        def op(b):
            dx = b.out((rows, cols), F32, pad=12, init=dx0 if acc else None, name="dx")
            dg, db = b.out((1, cols), name="dgamma"), b.out((1, cols), name="dbeta")
            xh = b.ws(rows * cols * 4, name="xhat_ws")
            capi.layernorm_bwd(b.inp(x.detach().float(), pad=4, name="x"), b.inp(gam.detach().float()), b.inp(dy, pad=8, name="dy"), dx,
                               dg, db, xh, accumulate_dx=acc)
            return {"dx": dx, "dgamma": dg, "dbeta": db}
        # 2e-5 + 1e-5 |ref| (test_layernorm_and_gelu_backward); the column sums run over `rows` terms in f32
        verify(*both(op), {"dx": (x.grad + (dx0.double() if acc else 0), 2e-5, 1e-5), "dgamma": (gam.grad, 2e-5 * max(1, rows ** 0.5), 1e-5),
                           "dbeta": (bet.grad, 2e-5 * max(1, rows ** 0.5), 1e-5)}, msg=f"layernorm_bwd acc={acc}")


# ---- dfd_gemm: the general 128x128 kernel -------------------------------------------------------------------------

def _gelu_q(u):
    return u * torch.sigmoid(1.702 * u)


@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("N", [5, 8, 200, 257])
@pytest.mark.parametrize("M", [1, 5, 129])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gemm_general_path(capi, M, N, K, dtype):
    """Scalar stores: any ldc >= N is admitted, so ldc = N + 1 (rows of C not even 8-byte aligned); lda, ldw = K + 8."""
    a, w = rnd(M, K, seed=8).to(dtype), rnd(N, K, seed=9, scale=K ** -0.5).to(dtype)
    bias = rnd(N, seed=10, scale=0.1)
    prod = a.double() @ w.double().T
    rt = 1e-5 if dtype == F32 else RT16
    LD = dict(lda=8, ldw=8, ldc=1)

    def run(epi, cdtype, ref, atol, rtol, use_bias=True, init=None, **kw):
        def op(b):
            c = b.out((M, N), cdtype, pad=LD["ldc"], init=init, name="C")
            capi.gemm(b.inp(a, pad=LD["lda"], name="A"), b.inp(w, pad=LD["ldw"], name="W"), c, b.inp(bias, name="bias") if use_bias else None, epi, **kw)
            assert capi.gemm_last_path() == 128
            return {"C": c}
        verify(*both(op), {"C": (ref, atol, rtol)}, msg=f"gemm128 epi {epi} bias={use_bias} C={cdtype}")

    for use_bias in (True, False):
        ref = prod + (bias.double() if use_bias else 0)
        run(capi.EPI_BIAS, dtype, ref, 1e-4, rt, use_bias)
        run(capi.EPI_BIAS_QUICKGELU, dtype, _gelu_q(ref), 1e-4, rt, use_bias)
        run(capi.EPI_BIAS_GELU, dtype, F.gelu(ref), 1e-4, rt, use_bias)
        x0 = rnd(M, N, seed=11)
        run(capi.EPI_BIAS_RESIDUAL, F32, x0.double() + ref, 2e-4, 1e-5, use_bias, init=x0)
    if dtype == BF16:
        run(capi.EPI_BIAS, F32, prod + bias.double(), 1e-4, 1e-5)
        with pytest.raises(capi.DfdError):  # the read-modify-write epilogues of the f32 residual stream need an f32 C
            capi.gemm(a.cuda(), w.cuda(), torch.zeros(M, N, device="cuda", dtype=BF16), None, capi.EPI_BIAS_RESIDUAL)

    # RESIDUAL_POS: separate strided residual, and in place; rows per frame = tokens - 1
    rows_pf, T = (M if M < 129 else 43), 2
    pos = rnd(T, N, seed=12)
    res = rnd(M, N, seed=13).to(dtype)
    frame = (torch.arange(M) // rows_pf) % T
    ref = res.double() + prod + pos[frame].double()
    for in_place in (False, True):
        def op(b):
            c = b.out((M, N), dtype, pad=1, init=res if in_place else None, name="C")
            capi.gemm(b.inp(a, pad=8), b.inp(w, pad=8), c, None, capi.EPI_RESIDUAL_POS, pos=b.inp(pos, name="pos"), tokens=rows_pf + 1,
                      frames_per_clip=T, residual=None if in_place else b.inp(res, pad=1, name="residual"))
            assert capi.gemm_last_path() == 128
            return {"C": c}
        verify(*both(op), {"C": (ref, 2e-4 if dtype == F32 else 1e-4, rt)}, msg=f"gemm128 residual_pos in_place={in_place}")

    # PATCH_EMBED (f32 token matrix): M patch rows of P per frame -> frames * (P + 1) token rows
    P_ = M if M < 129 else 43
    frames, tokens = M // P_, P_ + 1
    cls, tpos = rnd(N, seed=14), rnd(tokens, N, seed=15)
    want = torch.cat([cls.double().view(1, 1, N).expand(frames, 1, N), prod.view(frames, P_, N)], dim=1) + tpos.double()

    def op(b):
        c = b.out((frames * tokens, N), F32, pad=1, name="tokens")
        capi.gemm(b.inp(a, pad=8), b.inp(w, pad=8), c, None, capi.EPI_PATCH_EMBED, pos=b.inp(tpos), cls=b.inp(cls), tokens=tokens)
        assert capi.gemm_last_path() == 128
        return {"C": c}
    verify(*both(op), {"C": (want, 2e-4 if dtype == F32 else 2e-3, 0.0)}, msg="gemm128 patch_embed")

    # QKV_EXPORT: [q|k|v] needs N % 3 == 0, the [k|v] form N % 2 == 0, M a whole number of frames
    tok = M if M < 129 else 43
    blocks = 3 if N % 3 == 0 else 2 if N % 2 == 0 else 0
    if tok < 2 or blocks == 0:
        with pytest.raises(capi.DfdError):
            capi.gemm(a.cuda(), w.cuda(), torch.zeros(M, N, device="cuda", dtype=dtype), bias.cuda(), capi.EPI_QKV_EXPORT,
                      tokens=max(tok, 2), k_export=torch.zeros(M, N, device="cuda", dtype=dtype),
                      v_export=torch.zeros(M, N, device="cuda", dtype=dtype))
        return
    n_fr, D, T = M // tok, N // blocks, 2
    epos = rnd(T, D, seed=16)
    full = prod + bias.double()
    fv = full.view(n_fr, tok, blocks, D)
    pos_f = epos[torch.arange(n_fr) % T].view(n_fr, 1, D).double()

    def op(b):
        c = b.out((M, N), dtype, pad=1, name="C")
        ke = b.out((n_fr * (tok - 1), D), dtype, name="k_export")  # exactly frames * (tokens - 1) rows
        ve = b.out((n_fr * (tok - 1), D), dtype, name="v_export")
        capi.gemm(b.inp(a, pad=8), b.inp(w, pad=8), c, b.inp(bias), capi.EPI_QKV_EXPORT, pos=b.inp(epos), k_export=ke, v_export=ve,
                  tokens=tok, frames_per_clip=T, qkv_first=1 if blocks == 2 else 0)
        assert capi.gemm_last_path() == 128
        return {"C": c, "k": ke, "v": ve}
    verify(*both(op), {"C": (full, 1e-4, rt), "k": (fv[:, 1:, blocks - 2] + pos_f, 1e-4, rt), "v": (fv[:, 1:, blocks - 1] + pos_f, 1e-4, rt)},
           msg="gemm128 qkv export")


# ---- dfd_gemm: the tuned 256x256 kernels --------------------------------------------------------------------------

TUNED_NK = [(256, 384), (768, 768), (2304, 768), (768, 192), (1024, 640)]
TUNED_M = [1024 + 256 * 7 + 77, 1024 + 1]


def _family(path):
    return 256 if path in (256, 257) else path


def _tuned_operands(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + N * 7 + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(BF16)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    return g, a, w, bias


@pytest.mark.parametrize("N,K", TUNED_NK)
@pytest.mark.parametrize("M", TUNED_M)
def test_gemm_tuned_paths(capi, M, N, K):
    """lda = K + 8, ldw = K + 64 (rows of W stay 128-byte multiples: the ping-pong kernel remains eligible), ldc = N + 8."""
    g, a, w, bias = _tuned_operands(M, N, K)
    prod = a.double() @ w.double().T
    ref = prod + bias.double()
    pingpong = K % 128 == 0 and K >= 384 and N % 256 == 0
    paths, kernels = {}, {}

    def run(tag, epi, cdtype, want, atol, rtol, init=None, expect=None, use_bias=True, **kw):
        def op(b):
            c = b.out((M, N), cdtype, pad=8, init=init, name="C")
            capi.gemm(b.inp(a, pad=8, name="A"), b.inp(w, pad=64, name="W"), c, b.inp(bias, name="bias") if use_bias else None, epi, **kw)
            paths.setdefault(tag, []).append(capi.gemm_last_path())
            kernels.setdefault(tag, []).append(capi.gemm_last_kernel())
            return {"C": c}
        d, gg = both(op)
        pd, pg = paths[tag]
        if expect is not None:
            assert (pd, pg) == (expect, expect), f"{tag}: paths {pd} (dense) / {pg} (guarded), expected {expect}"
            # 256 is two kernels: the persistent one has the bf16 C, the one-workgroup-per-tile one the f32 C
            kernel = capi.GEMM_PINGPONG if expect == 257 else capi.GEMM_TILE if cdtype == F32 else capi.GEMM_PERSISTENT
            assert kernels[tag] == [kernel, kernel], f"{tag}: kernels {kernels[tag]}, expected {kernel}"
        verify(d, gg, {"C": (want, atol, rtol)}, same=_family(pd) == _family(pg), msg=f"tuned {tag} paths {pd}/{pg}")

    run("bias", capi.EPI_BIAS, BF16, ref, 1e-4, RT16, expect=257 if pingpong else 256)
    run("bias none", capi.EPI_BIAS, BF16, prod, 1e-4, RT16, expect=257 if pingpong else 256, use_bias=False)
    run("quickgelu", capi.EPI_BIAS_QUICKGELU, BF16, _gelu_q(ref), 1e-4, RT16, expect=257 if pingpong else 256)
    run("gelu", capi.EPI_BIAS_GELU, BF16, F.gelu(ref), 1e-4, RT16)
    run("bias f32 out", capi.EPI_BIAS, F32, ref, 1e-4, 1e-5, expect=256)
    x0 = torch.randn(M, N, device="cuda", generator=g)
    run("residual", capi.EPI_BIAS_RESIDUAL, F32, x0.double() + ref, 2e-4, 1e-5, init=x0, expect=256)
    run("stream_out", capi.EPI_BIAS_QUICKGELU, BF16, _gelu_q(ref), 1e-4, RT16, stream_out=True)
    run("tile_blocks=7", capi.EPI_BIAS, BF16, ref, 1e-4, RT16, tile_blocks=7)

    # RESIDUAL_POS: a separate strided residual, and in place
    P_, T_ = 16, 3
    res = torch.randn(M, N, device="cuda", generator=g).to(BF16)
    pos = torch.randn(T_, N, device="cuda", generator=g)
    frame = (torch.arange(M, device="cuda") // P_) % T_
    want = res.double() + prod + pos[frame].double()
    for in_place in (False, True):
        def op(b):
            c = b.out((M, N), BF16, pad=8, init=res if in_place else None, name="C")
            capi.gemm(b.inp(a, pad=8), b.inp(w, pad=64), c, None, capi.EPI_RESIDUAL_POS, pos=b.inp(pos, name="pos"), tokens=P_ + 1, frames_per_clip=T_,
                      residual=None if in_place else b.inp(res, pad=8, name="residual"))
            paths.setdefault(("rp", in_place), []).append(capi.gemm_last_path())
            return {"C": c}
        d, gg = both(op)
        pd, pg = paths[("rp", in_place)]
        assert _family(pd) == _family(pg) == 256, (pd, pg)
        verify(d, gg, {"C": (want, 1e-4, RT16)}, msg=f"tuned residual_pos in_place={in_place} paths {pd}/{pg}")

    # PATCH_EMBED with the m= override: the patch buffer is padded to whole 256-row tiles and its spare rows are poison
    P_ = 263 if M == 2893 else 41
    frames, tokens = M // P_, P_ + 1
    assert frames * P_ == M
    cls, tpos = torch.randn(N, device="cuda", generator=g), torch.randn(tokens, N, device="cuda", generator=g)
    want = torch.cat([cls.double().view(1, 1, N).expand(frames, 1, N), prod.view(frames, P_, N)], dim=1) + tpos.double()
    Mpad = (M + 255) // 256 * 256

    def op(b):
        ap = b.out((Mpad, K), BF16, pad=8, name="patches")
        ap[:M] = a
        if b.guard:
            b.items[-1][0].set(ap)  # an input from here on: re-take the snapshot
            b.items[-1] = (b.items[-1][0], True)
        c = b.out((frames * tokens, N), F32, pad=8, name="tokens")
        capi.gemm(ap, b.inp(w, pad=64), c, None, capi.EPI_PATCH_EMBED, m=M, pos=b.inp(tpos), cls=b.inp(cls), tokens=tokens)
        paths.setdefault("pe", []).append(capi.gemm_last_path())
        return {"C": c}
    d, gg = both(op)
    assert paths["pe"] == [256, 256], paths["pe"]
    verify(d, gg, {"C": (want, 2e-4, 1e-5)}, msg="tuned patch_embed")

    # QKV_EXPORT, export buffers of exactly frames * (tokens - 1) rows; then the [k|v] form on a column slice of C
    if N % 3 == 0 and (N // 3) % 256 == 0:
        tok = 263 if M == 2893 else 41
        n_fr, D, T = M // tok, N // 3, 3
        epos = torch.randn(T, D, device="cuda", generator=g)
        fv = ref.view(n_fr, tok, 3, D)
        pos_f = epos[torch.arange(n_fr, device="cuda") % T].view(n_fr, 1, D).double()
        for first in (0, 1):
            def op(b):
                c = b.out((M, N), BF16, pad=8, name="C")
                ke = b.out((n_fr * (tok - 1), D), BF16, name="k_export")
                ve = b.out((n_fr * (tok - 1), D), BF16, name="v_export")
                wv, bv = b.inp(w, pad=64, name="W"), b.inp(bias, name="bias")
                capi.gemm(b.inp(a, pad=8), wv[first * D:], c[:, first * D:], bv.reshape(-1)[first * D:], capi.EPI_QKV_EXPORT, pos=b.inp(epos),
                          k_export=ke, v_export=ve, tokens=tok, frames_per_clip=T, qkv_first=first)
                paths.setdefault(("qkv", first), []).append(capi.gemm_last_path())
                return {"C": c[:, first * D:], "q": c[:, :first * D], "k": ke, "v": ve}
            d, gg = both(op)
            pd, pg = paths[("qkv", first)]
            assert (pd, pg) == ((257, 257) if pingpong else (256, 256)), (pd, pg)
            for run_ in (d, gg):
                assert first == 0 or torch.isnan(run_.pop("q").float()).all(), "the query block must not be written"
                run_.pop("q", None)
            verify(d, gg, {"C": (ref[:, first * D:], 1e-4, RT16), "k": (fv[:, 1:, 1] + pos_f, 1e-4, RT16), "v": (fv[:, 1:, 2] + pos_f, 1e-4, RT16)},
                   msg=f"tuned qkv export qkv_first={first}")


def test_gemm_tuned_ldw_fallback(capi):
    """ldw = K + 8: rows of W are no longer 128-byte multiples, the ping-pong kernel declines and the round-2 persistent
    kernel (path 256) must give the bits of the dense call's ping-pong run."""
    M, N, K = 1024 + 256 * 7 + 77, 768, 768
    g, a, w, bias = _tuned_operands(M, N, K)
    ref = a.double() @ w.double().T + bias.double()
    paths = []

    def op(b):
        c = b.out((M, N), BF16, pad=8, name="C")
        capi.gemm(b.inp(a, pad=8), b.inp(w, pad=8), c, b.inp(bias), capi.EPI_BIAS_QUICKGELU)
        paths.append((capi.gemm_last_path(), capi.gemm_last_kernel()))
        return {"C": c}
    d, gg = both(op)
    assert paths == [(257, capi.GEMM_PINGPONG), (256, capi.GEMM_PERSISTENT)], paths
    verify(d, gg, {"C": (_gelu_q(ref), 1e-4, RT16)}, msg="ldw = K + 8")


# ---- dfd_gemm_fp8 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K,tok", [(2893, 768, 768, 263), (1024 + 96, 3072, 1024, 7)])
def test_gemm_fp8(capi, M, N, K, tok):
    """lda = K + 16, ldw = K + 128 (W rows stay 128-byte multiples), ldc = N + 8 (bf16) / N + 16 (e4m3).  Tolerances:
    test_gemm_fp8_epilogues (2^-11 of sum|a_k w_k| per element for the instruction's aligned accumulation)."""
    g = torch.Generator().manual_seed(N * 3 + K)
    a8 = (torch.randn(M, K, generator=g) * 4.0).to(E4M3)
    w8 = (torch.randn(N, K, generator=g) * 8.0).to(E4M3)
    af, wf = a8.double().cuda(), w8.double().cuda()
    cs = torch.rand(N, generator=g) * 0.02 + 0.001
    bias = torch.randn(N, generator=g) * 0.1
    ref = (af @ wf.T) * cs.double().cuda() + bias.double().cuda()
    AT = 2.0 ** -11 * (af.abs() @ wf.abs().T) * cs.double().cuda() + 1e-4
    gelu = _gelu_q(ref)
    out_scale = float(gelu.abs().max()) / 448.0

    def run(tag, epi, cdtype, want, atol, rtol, **kw):
        def op(b):
            c = b.out((M, N), cdtype, pad=8 if cdtype == BF16 else 16, name="C")
            capi.gemm_fp8(b.inp(a8, pad=16, name="A"), b.inp(w8, pad=128, name="W"), c, b.inp(cs, name="col_scale").reshape(-1), b.inp(bias, name="bias"), epi, **kw)
            return {"C": c}
        d, gg = both(op)
        for r_ in (d, gg):
            got = _f(r_["C"]) * (out_scale if cdtype == E4M3 else 1.0)
            assert torch.isfinite(got).all(), f"fp8 {tag}: non-finite"
            assert ((got - want).abs() <= atol + rtol * want.abs()).all(), f"fp8 {tag}: max err {(got - want).abs().max().item():.3e}"
        same_bits(d["C"], gg["C"], f"fp8 {tag}")

    run("bias", capi.EPI_BIAS, BF16, ref, AT, RT16)
    run("quickgelu", capi.EPI_BIAS_QUICKGELU, BF16, gelu, 1.1 * AT, RT16)
    run("quickgelu -> e4m3", capi.EPI_BIAS_QUICKGELU, E4M3, gelu, 1.1 * AT + 2.0 ** -10 * out_scale, 2 ** -4, out_inv_scale=1.0 / out_scale)
    run("bias -> e4m3", capi.EPI_BIAS, E4M3, ref.clamp(-448 * out_scale, 448 * out_scale), AT + 2.0 ** -10 * out_scale, 2 ** -4, out_inv_scale=1.0 / out_scale)

    n_fr, D, T = M // tok, N // 3, 3
    assert n_fr * tok == M
    epos = torch.randn(T, D, generator=g)
    fv, av = ref.view(n_fr, tok, 3, D), AT.view(n_fr, tok, 3, D)
    pos_f = epos.cuda()[torch.arange(n_fr, device="cuda") % T].view(n_fr, 1, D).double()

    def op(b):
        c = b.out((M, N), BF16, pad=8, name="C")
        ke = b.out((n_fr * (tok - 1), D), BF16, name="k_export")
        ve = b.out((n_fr * (tok - 1), D), BF16, name="v_export")
        capi.gemm_fp8(b.inp(a8, pad=16), b.inp(w8, pad=128), c, b.inp(cs).reshape(-1), b.inp(bias), capi.EPI_QKV_EXPORT, pos=b.inp(epos), k_export=ke,
                      v_export=ve, tokens=tok, frames_per_clip=T)
        return {"C": c, "k": ke, "v": ve}
    d, gg = both(op)
    for r_ in (d, gg):
        for name, want, at in (("C", ref, AT), ("k", fv[:, 1:, 1] + pos_f, av[:, 1:, 1]), ("v", fv[:, 1:, 2] + pos_f, av[:, 1:, 2])):
            got = r_[name].double().view(want.shape)
            assert torch.isfinite(got).all(), f"fp8 export {name}: non-finite"
            assert ((got - want).abs() <= at + RT16 * want.abs()).all(), f"fp8 export {name}"
    for name in d:
        same_bits(d[name], gg[name], f"fp8 export {name}")


# ---- dfd_gemm_at_b ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Ma,Nb", [(40, 8, 12), (777, 128, 32), (5000, 256, 768), (1600, 128, 128), (1601, 384, 640), (1600, 256, 256)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gemm_at_b(capi, R, Ma, Nb, dtype):
    """R not a multiple of 32, lda = Ma + 8, ldb = Nb + 8 (multiples of 8: the same kernel family as the dense call),
    the workspace exactly dfd_gemm_at_b_workspace(...) bytes.  The last three: the 128-wide tile of gemm_tn.hip, and an
    empty last split on either tile width (tests/test_hip_gemm_exact.py)."""
    a, bm = rnd(R, Ma, seed=40).to(dtype), rnd(R, Nb, seed=41).to(dtype)
    want = a.double().T @ bm.double()
    nbytes = capi.gemm_at_b_workspace_bytes(R, Ma, Nb, dtype)

    def op(b):
        c = b.out((Ma, Nb), F32, name="C")
        capi.gemm_at_b(b.inp(a, pad=8, name="A"), b.inp(bm, pad=8, name="B"), c, b.ws(nbytes))
        return {"C": c}
    verify(*both(op), {"C": (want, 1e-3 * R ** 0.5, 1e-4)}, msg="gemm_at_b")


# ---- dfd_attention_fwd --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tokens,heads", [(1, 1, 1), (2, 5, 2), (3, 197, 4), (64, 197, 12), (1, 257, 2), (40, 257, 16), (47, 230, 12)])
@pytest.mark.parametrize("dtype,out_pad", [(F32, 8), (BF16, 8), (F32, 4)])
def test_attention_fwd(capi, n, tokens, heads, dtype, out_pad):
    """ld_qkv = 3D + 8, ld_out = D + 8 (f32 also D + 4); the last frame's last row ends at the row padding and guard.
    The per-item and the persistent kernels are one family (pinned bit-identical by test_hip_kernels.py); the padded
    rows do not change which kernel serves the call."""
    D = heads * 64
    qkv = rnd(n * tokens, 3 * D, seed=16)
    qkv[:, :D] *= 2.0
    qkv = qkv.to(dtype)
    t = qkv.double().view(n, tokens, 3, heads, 64)
    aff = torch.einsum("nqhc,nkhc->nqkh", t[:, :, 0] / 8.0, t[:, :, 1]).softmax(dim=-2)
    want = torch.einsum("nqlh,nlhc->nqhc", aff, t[:, :, 2]).reshape(n * tokens, D)

    paths = []

    def op(b):
        out = b.out((n * tokens, D), dtype, pad=out_pad, name="out")
        capi.attention_fwd(b.inp(qkv, pad=8, name="qkv"), out, n, tokens, heads)
        paths.append(capi.attention_last_path())
        return {"out": out}
    tol = (2e-5, 1e-5) if dtype == F32 else (2e-2, 2 ** -7)
    verify(*both(op), {"out": (want, *tol)}, msg="attention")
    assert len(paths) == 2 and paths[0] == paths[1] != 0, f"dense and guarded call took kernels {paths}"
    assert paths[0] == capi.attention_plan(dtype, n, tokens, heads, n_cu=0).path


# ---- decoder and head kernels -------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 9, 64])
@pytest.mark.parametrize("N", [7, 101])
def test_linear_rows(capi, B, N):
    """Odd N and an odd ldy = N + 1 (scalar stores); ldx = K + 4."""
    K = 132
    x, w, bias = rnd(B, K, seed=20), rnd(N, K, seed=21, scale=K ** -0.5), rnd(N, seed=22, scale=0.1)
    ref = x.double() @ w.double().T + bias.double()
    y0 = rnd(B, N, seed=23)
    for epi, want, use_bias in ((capi.EPI_BIAS, ref, True), (capi.EPI_BIAS, ref - bias.double(), False), (capi.EPI_BIAS_QUICKGELU, _gelu_q(ref), True),
                                (capi.EPI_BIAS_RESIDUAL, y0.double() + ref, True)):
        def op(b):
            y = b.out((B, N), F32, pad=1, init=y0 if epi == capi.EPI_BIAS_RESIDUAL else None, name="y")
            capi.linear_rows(b.inp(x, pad=4, name="x"), b.inp(w, name="W"), b.inp(bias, name="bias") if use_bias else None, y, epi)
            return {"y": y}
        verify(*both(op), {"y": (want, 2e-5, 1e-5)}, msg=f"linear_rows epi {epi}")


@pytest.mark.parametrize("B", [1, 9, 64])
@pytest.mark.parametrize("N,K", [(8, 33), (100, 132), (260, 7)])
def test_linear_rows_t(capi, B, N, K):
    """N % 4 == 0 is the ABI's demand; K odd and below one 8-row step; ldx = K + 1, ldy = N + 4, ldr = N + 8; exact workspace."""
    x, w, bias = rnd(B, K, seed=28), rnd(N, K, seed=29, scale=K ** -0.5), rnd(N, seed=30, scale=0.1)
    ref = x.double() @ w.double().T + bias.double()
    y0 = rnd(B, N, seed=31)
    nbytes = capi.linear_rows_t_workspace_bytes(B, N, K)
    for tag, epi, want in (("bias", capi.EPI_BIAS, ref), ("quickgelu", capi.EPI_BIAS_QUICKGELU, _gelu_q(ref)),
                           ("residual in place", capi.EPI_BIAS_RESIDUAL, y0.double() + ref), ("residual", capi.EPI_BIAS_RESIDUAL, y0.double() + ref)):
        def op(b):
            y = b.out((B, N), F32, pad=4, init=y0 if tag == "residual in place" else None, name="y")
            capi.linear_rows_t(b.inp(x, pad=1, name="x"), b.inp(w.T.contiguous(), name="Wt"), b.inp(bias, name="bias").reshape(-1), y, b.ws(nbytes), epi,
                               residual=b.inp(y0, pad=8, name="residual") if tag == "residual" else None)
            return {"y": y}
        verify(*both(op), {"y": (want, 2e-5, 1e-5)}, msg=f"linear_rows_t {tag}")


@pytest.mark.parametrize("B", [1, 9, 64])
@pytest.mark.parametrize("N", [7, 101])
def test_linear_rows_bwd_weight(capi, B, N):
    K = 132
    x, dy = rnd(B, K, seed=5), rnd(B, N, seed=7)
    for with_db in (True, False):
        def op(b):
            dw = b.out((N, K), F32, name="dW")
            db = b.out((1, N), F32, name="db") if with_db else None
            capi.linear_rows_bwd_weight(b.inp(dy, pad=1, name="dy"), b.inp(x, pad=4, name="x"), dw, db)
            return {"dW": dw, "db": db} if with_db else {"dW": dw}
        refs = {"dW": (dy.double().T @ x.double(), 2e-5, 1e-5)}
        if with_db:
            refs["db"] = (dy.double().sum(0), 2e-5, 1e-5)
        verify(*both(op), refs, msg="linear_rows_bwd_weight")


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 101), (1537, 33), (32, 64)])
def test_transpose(capi, rows, cols):
    src = rnd(rows, cols, seed=6)

    def op(b):
        dst = b.out((cols, rows), F32, name="dst")
        capi.transpose(b.inp(src, name="src"), dst)
        return {"dst": dst}
    d, g = both(op)
    verify(d, g, {"dst": (src.T.double(), 0.0, 0.0)}, msg="transpose")


@pytest.mark.parametrize("B", [1, 9, 64])
@pytest.mark.parametrize("D,od", [(132, 7), (768, 2), (260, 101)])
def test_head(capi, B, D, od):
    """head_fwd with ldx = D + 4 (no multiple is demanded of ldx; the rows stay 16-byte aligned), then head_bwd."""
    x, gam, bet = rnd(B, D, seed=24, scale=2.0), 1 + 0.1 * rnd(D, seed=25), 0.1 * rnd(D, seed=26)
    proj = rnd(D, od, seed=27, scale=D ** -0.5)
    feat_ref = F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-5)
    z = feat_ref @ proj.double()

    def op(b):
        feat, raw, logits = b.out((B, D), name="feature"), b.out((B, od), name="raw"), b.out((B, od), name="logits")
        capi.head_fwd(b.inp(x, pad=4, name="x"), b.inp(gam), b.inp(bet), b.inp(proj, name="proj"), feat, raw, logits)
        return {"feat": feat, "raw": raw, "logits": logits}
    verify(*both(op), {"feat": (feat_ref, 2e-5, 0.0), "raw": (z, 2e-5, 1e-5), "logits": (ref_cpu.normalise_logits(z), 5e-5, 1e-5)}, msg="head_fwd")

    feat = rnd(B, D, seed=15).double().requires_grad_(True)
    pj = proj.double().requires_grad_(True)
    dl, dfe = rnd(B, od, seed=17), rnd(B, D, seed=18)
    zz = feat @ pj
    ((ref_cpu.normalise_logits(zz) * dl.double()).sum() + (feat * dfe.double()).sum()).backward()
    for ext in (True, False):
        def op(b):
            dz, df, dp = b.out((B, od), name="dz"), b.out((B, D), name="dfeat"), b.out((D, od), name="dproj")
            capi.head_bwd(b.inp(zz.detach().float(), name="raw"), b.inp(dl), b.inp(proj), b.inp(feat.detach().float(), name="feat"),
                          b.inp(dfe, name="dfeat_ext") if ext else None, dz, df, dp)
            return {"dfeat": df, "dproj": dp, "dz": dz}
        verify(*both(op), {"dfeat": (feat.grad - (0 if ext else dfe.double()), 2e-5, 1e-4), "dproj": (pj.grad, 2e-5, 1e-4)}, msg="head_bwd")


@pytest.mark.parametrize("modes", [0, 2, 3])
@pytest.mark.parametrize("B,T,P,heads", [(1, 1, 1, 1), (9, 3, 101, 2), (64, 2, 7, 4)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decoder_attention(capi, B, T, P, heads, dtype, modes):
    """Keys / values read in place from a q|k|v activation [frames, tokens, 3D] whose rows carry 8 elements of padding, with
    its CLS rows and its whole query block poisoned (the decoder must skip them), the temporal positional embedding added
    on the fly; forward, attn_mode forward / backward and backward with dK / dV, every workspace of the exact size."""
    D, S, tok = heads * 64, T * P, P + 1
    k = rnd(B, S, heads, 64, seed=1).to(dtype).float()
    v = rnd(B, S, heads, 64, seed=2).to(dtype).float()
    q = rnd(B, 1, heads, 128, seed=3).requires_grad_(True)
    pos = (0.3 * rnd(T, 1, heads, 64, seed=4)).requires_grad_(True)
    m = torch.ones(B, T, dtype=torch.bool)
    if B > 1 and modes in (0, 2) and T > 1:  # "frame" groups of a padded frame are NaN, in the reference as well
        m[1, T - 1:] = False
    attn_mode = tuple(nm for nm, bit in (("frame", 1), ("temporal", 2)) if modes & bit)
    w = {"p.attn.in_proj.weight": torch.eye(2 * D), "p.attn.in_proj.bias": torch.zeros(2 * D),
         "p.attn.out_proj.weight": torch.eye(D), "p.attn.out_proj.bias": torch.zeros(D)}
    kk = (k.view(B, T, P, heads, 64) + pos).flatten(1, 2).requires_grad_(True)
    vv = (v.view(B, T, P, heads, 64) + pos).flatten(1, 2).requires_grad_(True)
    kk.retain_grad(), vv.retain_grad()
    kw = dict(attn_mode=attn_mode) if modes else {}
    out = ref_cpu.decoder_attention(q.reshape(B, 1, 2 * D), kk, vv, m.repeat_interleave(P, dim=-1), w, "p.", heads, T, **kw)
    dmix = rnd(B, D, seed=5)
    (out.reshape(B, D) * dmix).sum().backward()

    qkv = torch.full((B * T, tok, 3 * D), float("nan"))
    qkv[:, 1:, D:2 * D] = k.reshape(B * T, P, D)
    qkv[:, 1:, 2 * D:] = v.reshape(B * T, P, D)
    qkv = qkv.to(dtype).reshape(B * T * tok, 3 * D)
    splits = 3
    posd = pos.detach().reshape(T, D)

    def op(b):
        a2 = b.inp(qkv, pad=8, name="qkv")
        a3 = a2.as_strided((B * T, tok, 3 * D), (tok * a2.stride(0), a2.stride(0), 1))
        kv_, vv_ = a3[:, 1:, D:2 * D], a3[:, 1:, 2 * D:]
        qd, md, pd = b.inp(q.detach().reshape(B, 2 * D), name="q"), b.inp(m.to(torch.uint8), fill=1, name="frame_mask"), b.inp(posd, name="pos")
        dm = b.inp(dmix, name="dmix")
        mix, mix_s, stats = b.out((B, D), name="mix"), b.out((B, D), name="mix_softmax"), b.out((B, heads * 2), name="stats")
        sc = aw = dsc = None
        if modes:
            sc, aw, dsc = b.out((B * heads, S), name="scores"), b.out((B * heads, S), name="weights"), b.out((B * heads, S), name="dscores")
            capi.decoder_attn_modes_fwd(qd, kv_, md, modes, sc, aw, B, T, P, heads, pos=pd)
        capi.decoder_attn_fwd(qd, kv_, vv_, md, mix, stats, b.ws(capi.decoder_attn_workspace_bytes(B, heads, 64, splits)), splits, B, T, P, heads,
                              mix_softmax=mix_s, ext_weights=aw, pos=pd)
        if modes:
            capi.decoder_attn_modes_bwd(sc, vv_, dm, modes, b.out((B * heads, S), name="dwv_workspace"), dsc, B, T, P, heads, pos=pd)
        dq, dpos = b.out((B, 2 * D), name="dq"), b.out((T, D), name="dpos")
        dk, dv = b.out((B * S, D), name="dk"), b.out((B * S, D), name="dv")
        capi.decoder_attn_bwd(qd, kv_, vv_, md, dm, None if modes else mix_s, None if modes else stats, dq, dpos,
                              b.ws(capi.decoder_attn_bwd_workspace_bytes(B, T, heads)), B, T, P, heads, dk=dk, dv=dv, ext_weights=aw, ext_dscores=dsc, pos=pd)
        r = {"mix": mix, "dq": dq, "dpos": dpos, "dk": dk, "dv": dv}
        if not modes:
            r["stats"], r["mix_softmax"] = stats, mix_s
        else:
            r["weights"] = aw
        return r
    scale = max(1.0, out.abs().max().item()) if modes else 1.0
    gs = max(1.0, q.grad.abs().max().item()) if modes else 1.0
    t_ = (5e-5, 5e-6, 1e-4) if modes else (2e-5, 2e-6, 5e-5)  # test_decoder_attention_modes / test_decoder_attention_backward
    verify(*both(op), {"mix": (out.reshape(B, D), 2e-5 * scale, 1e-4), "dq": (q.grad.reshape(B, 2 * D), t_[0] * gs, 2e-4),
                       "dk": (kk.grad.reshape(B * S, D), t_[1] * gs, 2e-4), "dv": (vv.grad.reshape(B * S, D), t_[1] * gs, 2e-4),
                       "dpos": (pos.grad.reshape(T, D), t_[2] * gs, 2e-4)}, msg=f"decoder attention modes={modes}")


# ---- contiguous-only kernels --------------------------------------------------------------------------------------

def _rng(seed, step):
    return torch.tensor([seed, step], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("n", [1, 8, 104, 1001])
@pytest.mark.parametrize("in_dtype,out_dtype", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)])
def test_dropout(capi, n, in_dtype, out_dtype):
    seed, step, site, p = 0x1234_5678_9ABC, 41, 7, 0.3
    x = rnd(n, seed=n).to(in_dtype)
    want = x.double() * torch.from_numpy(dropout_mask.multiplier(n, p, seed, step, site)).double()

    def op(b):
        y = b.out((1, n), out_dtype, name="out")
        capi.dropout(b.inp(x.view(1, n), name="in"), y, capi.Dropout(_rng(seed, step), site, p))
        return {"y": y}
    verify(*both(op), {"y": (want, 0.0, 1e-6 if out_dtype == F32 else RT16)}, msg="dropout")


@pytest.mark.parametrize("n", [1, 8, 104, 1001])
def test_quickgelu(capi, n):
    u = rnd(n, seed=13, scale=2.0).double().requires_grad_(True)
    du = rnd(n, seed=14)
    (ref_cpu.quick_gelu(u) * du.double()).sum().backward()
    for bwd in (False, True):
        def op(b):
            out = b.out((1, n), name="out")
            capi.quickgelu(b.inp(u.detach().float().view(1, n), name="u"), out, du=b.inp(du.view(1, n), name="du") if bwd else None)
            return {"out": out}
        verify(*both(op), {"out": (u.grad if bwd else ref_cpu.quick_gelu(u.detach()), 2e-6, 1e-5)}, msg=f"quickgelu bwd={bwd}")


@pytest.mark.parametrize("n", [8, 8 * 13, 8 * 1025])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_erf(capi, n, dtype):
    a = (3 * rnd(n, seed=5)).to(dtype)
    dh = rnd(n, seed=6).to(dtype)
    seed, step, site, p = 1234, 9, 77, 0.3
    mask = torch.from_numpy(dropout_mask.multiplier(n, p, seed, step, site)).double()
    ad = a.double().requires_grad_(True)
    hr = F.gelu(ad) * mask
    hr.backward(dh.double())
    tol = 2e-6 if dtype == F32 else RT16  # relative to the largest reference value (test_gelu_erf_kernels_against_f64)

    def op(b):
        drop = capi.Dropout(_rng(seed, step), site, p)
        av = b.inp(a.view(1, n), name="a")
        h, da = b.out((1, n), dtype, name="h"), b.out((1, n), dtype, name="da")
        capi.gelu_erf(av, h, drop)
        capi.gelu_erf_bwd(av, b.inp(dh.view(1, n), name="dh"), da, drop)
        return {"h": h, "da": da}
    verify(*both(op), {"h": (hr.detach(), tol * hr.detach().abs().max().item(), 0.0),
                       "da": (ad.grad, max(tol, 1e-5) * ad.grad.abs().max().item(), 0.0)}, msg="gelu_erf")


@pytest.mark.parametrize("frames,P,x", [(1, 1, 8), (3, 5, 72), (2, 7, 256)])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_adapter_norm_gelu(capi, frames, P, x, mode, dtype):
    a = rnd(frames, P, x, seed=50, scale=1.5).to(dtype).double().requires_grad_(True)
    shape = (P, x) if mode == 1 else (x,)
    w = (1 + 0.1 * rnd(*shape, seed=51)).double().requires_grad_(True)
    bb = (0.1 * rnd(*shape, seed=52)).double().requires_grad_(True)
    dy = rnd(frames, P, x, seed=53).to(dtype)
    y = F.layer_norm(F.gelu(a), shape, w, bb, 1e-5) if mode == 2 else F.gelu(F.layer_norm(a, shape, w, bb, 1e-5))
    (y * dy.double()).sum().backward()
    nbytes = capi.adapter_norm_gelu_bwd_workspace_bytes(frames, P, x, mode)

    def op(b):
        ad = b.inp(a.detach().to(dtype), name="a")
        wd, bd = b.inp(w.detach().float().reshape(1, -1), name="weight"), b.inp(bb.detach().float().reshape(1, -1), name="bias")
        yd, da = b.out((frames * P, x), dtype, name="y"), b.out((frames * P, x), dtype, name="da")
        dw, db = b.out((1, w.numel()), name="dweight"), b.out((1, w.numel()), name="dbias")
        capi.adapter_norm_gelu(ad, yd, wd, bd, frames, P, x, mode)
        capi.adapter_norm_gelu_bwd(ad, b.inp(dy, name="dy"), da, wd, bd, dw, db, b.ws(nbytes), frames, P, x, mode)
        return {"y": yd, "da": da, "dw": dw, "db": db}
    t0, r0 = (2e-5, 1e-3) if dtype == F32 else (2e-2, 2e-2)  # test_adapter_norm_gelu_backward
    ta = 1e-3 if dtype == F32 else 5e-2
    verify(*both(op), {"y": (y.detach(), t0, r0), "da": (a.grad, t0, r0), "dw": (w.grad, ta, 1e-3), "db": (bb.grad, ta, 1e-3)},
           msg=f"adapter_norm_gelu mode {mode}")


def _rel(got, ref, tol, msg):
    got, ref = _f(got).cpu().reshape(-1), ref.double().cpu().reshape(-1)
    assert torch.isfinite(got).all(), f"{msg}: non-finite"
    err = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
    assert err <= tol, f"{msg}: relative error {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("B,T,P,D", [(1, 1, 1, 8), (2, 3, 5, 72), (3, 2, 7, 768)])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("train", [True, False])
def test_adapter_bn(capi, B, T, P, D, dtype, train):
    """Tolerances: test_batchnorm_kernels_against_f64 (relative to the largest reference value)."""
    frames, rows = B * T, B * T * P
    y = (rnd(rows, D, seed=1) * 1.7 + 3.0).to(dtype)
    res, dout = rnd(rows, D, seed=2).to(dtype), rnd(rows, D, seed=3).to(dtype)
    pos, gamma, beta = rnd(T, D, seed=4), 1 + 0.1 * rnd(T, seed=5), 0.1 * rnd(T, seed=6)
    rm0, rv0 = 0.1 * rnd(T, seed=7), 0.5 + rnd(T, seed=8).abs()
    yd = y.double().view(B, T, P, D).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    z = F.batch_norm(yd, rm64, rv64, g64, b64, training=train, momentum=0.1, eps=1e-5)
    ref = res.double().view(B, T, P, D) + z + pos.double().view(1, T, 1, D)
    ref.backward(dout.double().view(B, T, P, D))
    mean = yd.detach().mean((0, 2, 3)) if train else rm0.double()
    var = yd.detach().var((0, 2, 3), unbiased=False) if train else rv0.double()
    nbytes = capi.adapter_bn_workspace_bytes(frames, P, D)
    mode = capi.BN_TRAIN_UPDATE if train else capi.BN_EVAL

    def op(b):
        yv = b.inp(y, name="y")
        stats = b.out((2, T), name="stats")
        rm, rv = b.out((1, T), init=rm0, name="running_mean"), b.out((1, T), init=rv0, name="running_var")
        nbt = torch.full((1,), 7, device="cuda", dtype=torch.int64)
        ws = b.ws(nbytes)
        capi.adapter_bn_stats(yv, stats, ws, frames, P, T, mode, rm, rv, nbt)
        out = b.out((rows, D), dtype, name="out")
        gv = b.inp(gamma.view(1, T), name="gamma")
        capi.adapter_bn_apply(yv, out, frames, P, T, stats, gv, b.inp(beta.view(1, T), name="beta"), residual=b.inp(res, name="residual"),
                              pos=b.inp(pos, name="pos"))
        dy, dg, db = b.out((rows, D), dtype, name="dy"), b.out((1, T), name="dgamma"), b.out((1, T), name="dbeta")
        capi.adapter_bn_bwd(yv, b.inp(dout, name="dout"), dy, stats, gv, dg, db, ws, frames, P, T, train)
        torch.cuda.synchronize()
        assert nbt.item() == (8 if train else 7)
        return {"stats": stats, "rm": rm, "rv": rv, "out": out, "dy": dy, "dg": dg, "db": db}
    d, g = both(op)
    for r_ in (d, g):
        _rel(r_["stats"][0], mean, 1e-5, "mean")
        _rel(r_["stats"][1], (var + 1e-5).rsqrt(), 1e-5, "invstd")
        _rel(r_["rm"], rm64, 1e-5, "running mean")
        _rel(r_["rv"], rv64, 1e-5, "running var")
        _rel(r_["out"], ref.detach(), 1e-5 if dtype == F32 else 2.0 ** -7, "out")
        _rel(r_["dg"], g64.grad, 1e-4, "dgamma")
        _rel(r_["db"], b64.grad, 1e-4, "dbeta")
        _rel(r_["dy"], yd.grad, 1e-4 if dtype == F32 else 2.0 ** -7, "dy")
    for name in d:
        same_bits(d[name], g[name], f"adapter_bn {name}")

    # the "linear" struct's epilogue: no statistics, no residual, f32 y
    def op(b):
        out = b.out((rows, D), dtype, name="out")
        capi.adapter_bn_apply(b.inp(y.float(), name="y"), out, frames, P, T, pos=b.inp(pos, name="pos"))
        return {"out": out}
    d, g = both(op)
    want = y.double().view(B, T, P, D) + pos.double().view(1, T, 1, D)
    for r_ in (d, g):
        _rel(r_["out"], want, 1e-5 if dtype == F32 else 2.0 ** -7, "linear epilogue")
    same_bits(d["out"], g["out"], "adapter_bn linear epilogue")


@pytest.mark.parametrize("B,L,P,T,D", [(2, 1, 1, 1, 8), (3, 2, 5, 3, 72), (5, 1, 7, 2, 768)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_compinv_loss(capi, B, L, P, T, D, dtype):
    """The smallest legal pair loss (B = 2, T = P = L = 1, D = 8) and ragged ones with an odd last clip; tolerances of
    test_loss_kernels_against_f64."""
    k, v = rnd(L, B * T * P, D, seed=1).to(dtype), rnd(L, B * T * P, D, seed=2).to(dtype)
    kd_, vd_ = k.double().requires_grad_(True), v.double().requires_grad_(True)
    wpairs, s = B // 2, 0
    for t in (kd_, vd_):
        a = t.view(L, B, T * P, D)
        s = s + (a[:, 0:2 * wpairs:2] - a[:, 1:2 * wpairs:2]).abs().sum((0, 1))
    Mr = (s / (wpairs * L * 2)).view(P, T, D).mean(1)
    match = Mr.norm() / P
    match.backward()
    nbytes = capi.compinv_loss_workspace_bytes(P, D)
    assert nbytes % 4 == 0 and nbytes >= P * D * 4

    def op(b):
        kv_, vv_ = b.inp(k, name="k"), b.inp(v, name="v")
        ws = b.ws(nbytes).view(torch.float32)
        mt, nm, rc = b.out((1, 1), name="match"), b.out((1, 1), name="norm"), b.out((1, 1), name="recon")
        capi.compinv_loss_fwd(kv_, vv_, B, T, P, ws, mt.view(()), nm.view(()), rc.view(()))
        dk, dv = b.out((L, B * T * P, D), dtype, name="dk"), b.out((L, B * T * P, D), dtype, name="dv")
        capi.compinv_loss_bwd(kv_, vv_, B, T, P, ws, nm.view(()), b.inp(torch.full((1, 1), 0.75), name="grad").view(1), dk, dv)
        torch.cuda.synchronize()
        return {"M": ws[:P * D].clone(), "match": mt, "norm": nm, "recon": rc, "dk": dk, "dv": dv}
    d, g = both(op)
    for r_ in (d, g):
        assert r_["recon"].item() == 0.0
        assert abs(r_["match"].item() - match.item()) <= 1e-5 * match.item()
        assert abs(r_["norm"].item() - match.item() * P) <= 1e-5 * match.item() * P
        assert (r_["M"].double().cpu().view(P, D) - Mr.detach()).abs().max().item() <= 1e-5 * Mr.abs().max().item()
        for got, ref in ((r_["dk"], kd_.grad * 0.75), (r_["dv"], vd_.grad * 0.75)):
            got = got.double().cpu()
            assert torch.isfinite(got).all()
            err = (got - ref).abs()
            if dtype == F32:
                assert err.max().item() <= 1e-5 * ref.abs().max().item()
            else:
                assert (err <= 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()).all()
    for name in d:
        same_bits(d[name], g[name], f"compinv {name}")


@pytest.mark.parametrize("n,res,patch,kpad", [(1, 4, 4, 48), (3, 32, 16, 768), (2, 28, 14, 640), (1, 15, 5, 76), (2, 64, 8, 192)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_patchify(capi, n, res, patch, kpad, dtype):
    """Both kernels: bf16 rows of 4-aligned patch sizes take the strip kernel, everything else the general one; pad columns
    (kpad > 3 * patch^2) must come out zero."""
    frames = rnd(n, 3, res, res, seed=41)
    P, kk = (res // patch) ** 2, 3 * patch * patch
    want = torch.zeros(n * P, kpad, dtype=torch.float64)
    want[:, :kk] = frames.view(n, 3, res // patch, patch, res // patch, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * P, kk).to(dtype).double()

    def op(b):
        out = b.out((n * P, kpad), dtype, name="patches")
        capi.patchify(b.inp(frames, name="frames"), out, res, patch)
        return {"out": out}
    verify(*both(op), {"out": (want, 0.0, 0.0)}, msg="patchify")


MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def _transform_ref(frames, res, antialias):
    """torchvision's Resize(res, BICUBIC) -> CenterCrop -> float -> Normalize, restated (tests/test_hip_preprocess.py)."""
    n, _, h, w = frames.shape
    s, l = (h, w) if h <= w else (w, h)
    new_l = int(res * l / s)
    nh, nw = (res, new_l) if h <= w else (new_l, res)
    x = frames.float()
    if (nh, nw) != (h, w):
        x = F.interpolate(x, size=(nh, nw), mode="bicubic", antialias=antialias, align_corners=False).round().clamp(0, 255)
    top, left = int(round((nh - res) / 2.0)), int(round((nw - res) / 2.0))
    x = x[..., top:top + res, left:left + res] / 255.0
    return (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)


@pytest.mark.parametrize("h,w,res,patch", [(16, 16, 16, 16), (32, 32, 32, 16), (45, 37, 32, 16), (97, 131, 28, 14)])
@pytest.mark.parametrize("patch_rows", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_preprocess_u8(capi, h, w, res, patch, patch_rows, dtype):
    """uint8 frames between guards of 255 (a pixel read outside the frames changes the result).  No resize: exact (2e-6);
    resized: within one uint8 level, at most 5e-4 of the pixels off at all (test_hip_preprocess.check)."""
    n = 3
    rng = np.random.default_rng(h * 1000 + w)
    low = torch.from_numpy(rng.uniform(0, 255, (n, 3, max(2, h // 16), max(2, w // 16))).astype(np.float32))
    frames = (F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
              + torch.from_numpy(rng.normal(0, 12, (n, 3, h, w)).astype(np.float32))).round().clamp(0, 255).to(torch.uint8)
    P, kk = (res // patch) ** 2, 3 * patch * patch
    kpad = (kk + 63) // 64 * 64
    for antialias in (False, True):
        want = _transform_ref(frames, res, antialias)
        if patch_rows:
            wp = torch.zeros(n * P, kpad)
            wp[:, :kk] = want.view(n, 3, res // patch, patch, res // patch, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * P, kk)
            want = wp

        def op(b):
            out = b.out((n * P, kpad) if patch_rows else (n, 3, res, res), dtype, name="out")
            capi.preprocess_u8(b.inp(frames, fill=255, name="frames"), out, res, patch, MEAN, STD, antialias=antialias, patch_rows=patch_rows)
            return {"out": out}
        d, g = both(op)
        for r_ in (d, g):
            got = r_["out"].float().cpu()
            assert torch.isfinite(got).all()
            err = (got - want.to(dtype).float()).abs()
            r16 = 0.0 if dtype == F32 else 2.0 ** -8 * 3.0  # one bf16 rounding of values up to ~2.7
            if (h, w) == (res, res):
                assert err.max().item() <= 2e-6 + r16
            else:
                level = (1.0 / 255.0) / min(STD)
                assert err.max().item() <= level * 1.001 + 2e-6 + r16
                assert int((err > 2e-6 + r16).sum()) <= max(1, 5e-4 * err.numel())
        same_bits(d["out"], g["out"], "preprocess_u8")


def test_sgd_step(capi):
    """Params, grads, velocities and mirrors each between guards; a mirrored [1537, 33] weight (ragged for the transposing
    tiles), the smallest entries (1 and 5 elements), two steps (first_step initialises the velocity).  Reference:
    torch.optim.SGD's arithmetic in f64; tolerance 1e-6 * max(1, |ref|) (test_fused_sgd_equals_torch_sgd_step_by_step)."""
    shapes = [((1537, 33), True), ((1,), False), ((5,), False), ((8, 7), True), ((2, 768), False)]
    lr, mom, wd = 0.01, 0.95, 0.01
    p0 = [rnd(*s, seed=60 + i) for i, (s, _) in enumerate(shapes)]
    gr = [[rnd(*s, seed=70 + 10 * st + i) for i, (s, _) in enumerate(shapes)] for st in range(2)]
    pr, br = [p.double() for p in p0], [None] * len(shapes)
    for st in range(2):
        for i in range(len(shapes)):
            gg = gr[st][i].double() + wd * pr[i]
            br[i] = gg if st == 0 else mom * br[i] + gg
            pr[i] = pr[i] - lr * br[i]

    def op(b):
        ps = [b.out((1, p.numel()), init=p, name=f"p{i}") for i, p in enumerate(p0)]
        gs = [b.out((1, p.numel()), init=gr[0][i], name=f"g{i}") for i, p in enumerate(p0)]
        bufs = [b.out((1, p.numel()), name=f"buf{i}") for i, p in enumerate(p0)]
        mirs = [b.out((s[1], s[0]), name=f"mirror{i}") if mir else None for i, (s, mir) in enumerate(shapes)]
        rows_, first = [], 0
        for i, (s, mir) in enumerate(shapes):
            r, c = (s[0], s[1]) if len(s) == 2 else (0, 0)
            rows_.append([ps[i].data_ptr(), gs[i].data_ptr(), bufs[i].data_ptr(), mirs[i].data_ptr() if mir else 0, p0[i].numel(), r | (c << 32), first])
            first += capi.sgd_blocks(p0[i].numel(), r, c, mir)
        table = torch.tensor(rows_, dtype=torch.int64, device="cuda")
        capi.sgd_step(table, len(shapes), first, lr, mom, wd, True)
        torch.cuda.synchronize()
        if b.guard:  # the gradients are inputs: nothing of them may change; then load the second step's
            for g_, _ in b.items:
                if g_.name.startswith("g"):
                    g_.assert_untouched(view_too=True)
        for i in range(len(shapes)):
            gs[i].copy_(gr[1][i].reshape(1, -1))
        if b.guard:
            for g_, _ in b.items:
                if g_.name.startswith("g"):
                    g_._snap = g_.flat.clone()
        capi.sgd_step(table, len(shapes), first, lr, mom, wd, False)
        out = {f"p{i}": ps[i] for i in range(len(shapes))}
        out.update({f"buf{i}": bufs[i] for i in range(len(shapes))})
        out.update({f"mirror{i}": mirs[i] for i, (_, mir) in enumerate(shapes) if mir})
        return out
    d, g = both(op)
    refs = {}
    for i, (s, mir) in enumerate(shapes):
        refs[f"p{i}"] = (pr[i], 1e-6 * max(1.0, pr[i].abs().max().item()), 0.0)
        refs[f"buf{i}"] = (br[i], 1e-6 * max(1.0, br[i].abs().max().item()), 0.0)
    verify(d, g, refs, msg="sgd_step")
    for r_ in (d, g):
        for i, (s, mir) in enumerate(shapes):
            if mir:
                assert torch.equal(r_[f"mirror{i}"], r_[f"p{i}"].view(s).t()), f"mirror {i} is not the transpose of the updated weight"
