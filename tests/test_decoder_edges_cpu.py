"""The references and tables of tests/decoder_edge_cases.py, checked without a GPU: the float64 restatement is the
oracle's decoder attention (forward and autograd), the tables hold what they promise, and the restated launch
geometry fits a workgroup."""
import pytest
import torch

from oracle import ref_cpu
from tests import decoder_edge_cases as dec
from tests.decoder_edge_cases import BARS, MASKS, SHAPES, deals, operands, reference, splits_for

SMALL = [s for s in SHAPES if s[1] * s[2] <= 200]


def oracle(o, mask, T, heads, attn_mode, dtype):
    """oracle.ref_cpu.decoder_attention with identity projections, as tests/test_hip_backward.py builds it"""
    B, S, D = o["k"].shape
    P = S // T
    q = o["q"].detach().to(dtype).reshape(B, 1, 2 * D).clone().requires_grad_(True)
    pos = torch.zeros(T, 1, heads, 64, dtype=dtype, requires_grad=True)
    w = {"p.attn.in_proj.weight": torch.eye(2 * D, dtype=dtype), "p.attn.in_proj.bias": torch.zeros(2 * D, dtype=dtype),
         "p.attn.out_proj.weight": torch.eye(D, dtype=dtype), "p.attn.out_proj.bias": torch.zeros(D, dtype=dtype)}
    kk = (o["k"].to(dtype).view(B, T, P, heads, 64) + pos).flatten(1, 2)
    vv = (o["v"].to(dtype).view(B, T, P, heads, 64) + pos).flatten(1, 2)
    kk.retain_grad(), vv.retain_grad()
    out = ref_cpu.decoder_attention(q, kk, vv, mask.repeat_interleave(P, dim=-1), w, "p.", heads, T, attn_mode=attn_mode)
    (out.reshape(B, D) * o["dmix"].to(dtype)).sum().backward()
    return dict(mix=out.detach().reshape(B, D), dq=q.grad.reshape(B, 2 * D), dk=kk.grad.reshape(B, S, D),
                dv=vv.grad.reshape(B, S, D), dpos=pos.grad.reshape(T, D))


@pytest.mark.parametrize("B,T,P,heads", SMALL)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restatement_is_the_oracle(B, T, P, heads, dtype):
    """Every small shape x mask-deal, plain and under attn_mode ("temporal" with every deal, the "frame" modes with full
    clips): the oracle evaluated in float64 is the restatement to 1e-10, and evaluated in float32 (as the GPU tests of
    the kernels evaluate it) it is within the project's kernel bars of it."""
    o = operands(B, T, P, heads, dtype)
    for names, mask in deals(B, T):
        for attn_mode in ((), ("temporal",), ("frame",), ("frame", "temporal")):
            if "frame" in attn_mode and not mask.all():
                continue
            want = reference(o, mask, T, attn_mode)
            for odt, bars in ((torch.float64, None), (torch.float32, BARS)):
                got = oracle(o, mask, T, heads, attn_mode, odt)
                for n, t in got.items():
                    scale = max(1.0, want["mix" if n == "mix" else "dq"].abs().max().item()) if attn_mode else 1.0
                    atol, rtol = (1e-10, 1e-10) if bars is None else (dec.MODES_BARS[n] if attn_mode else bars[n])
                    err, over = dec.worst(t, want[n], atol * scale, rtol)
                    assert over <= 0, f"{names} {attn_mode} {odt} {n}: worst error {err:.3e}"
            # the float32 evaluation of the restatement (what a missed bar is weighed against) is the same function
            f32 = reference(o, mask, T, attn_mode, dtype=torch.float32)
            f64 = dec._restate_in(torch.float64, o["q"].double(), o["k"].double(), o["v"].double(), mask, T, attn_mode)
            for n in ("mix", "mix_softmax", "max", "sumexp", "ws", "wc"):
                assert dec.worst(f64[n], want[n], 1e-12, 1e-12)[1] <= 0, n
                assert dec.worst(f32[n], want[n], 2e-5 * (max(1.0, want["mix"].abs().max().item()) if attn_mode else 1.0), 1e-4)[1] <= 0, n
    # the statistics and the weights are what they say
    want = reference(o, deals(B, T)[0][1], T)
    assert torch.allclose(want["ws"].sum(-1), torch.ones(B, heads, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(want["mix"], 0.5 * want["mix_softmax"] + 0.5 * torch.einsum(
        "bhs,bshc->bhc", want["wc"], o["v"].double().view(B, T * P, heads, 64)).reshape(B, -1), atol=1e-12)


def test_tables_are_well_formed():
    assert len(set(SHAPES)) == 7 and set(MASKS) == {"full", "tail", "head", "hole", "only_first", "only_last", "alternate"}
    for B, T, P, heads in SHAPES:
        S = T * P
        seen = set()
        for names, mask in deals(B, T):
            assert mask.shape == (B, T) and mask.dtype == torch.bool
            assert mask.any(dim=1).all(), f"{names}: a clip without a valid frame"
            seen.update(names)
            for b, n in enumerate(names):
                assert torch.equal(mask[b], dec.frame_mask(n, T))
        assert seen == (set(MASKS) if T > 1 else {"full"})
        if T >= 3:  # every pattern is itself and no other
            pats = {n: dec.frame_mask(n, T) for n in MASKS}
            assert pats["full"].all() and not pats["tail"][-1] and pats["tail"][0] and not pats["head"][0] and pats["head"][-1]
            assert pats["hole"][0] and pats["hole"][-1] and not pats["hole"].all()
            assert pats["only_first"].tolist() == [True] + [False] * (T - 1) and pats["only_last"].tolist() == [False] * (T - 1) + [True]
            assert pats["alternate"].tolist() == [t % 2 == 0 for t in range(T)]
        sp = splits_for(B, S)
        assert len(sp) == len(set(sp)) and all(1 <= s <= 4096 for s in sp)
        assert {1, 2, 3, 7, 65, 130, S, S + 1, 2 * S + 3, dec.policy_splits(B, S)} == set(sp)
        assert max(sp) > 64 and any(dec.empty_splits(S, s) > 0 for s in sp), "no empty split / no second trip of the combine loop"
        assert dec.empty_splits(S, S) == 0 and dec.empty_splits(S, 2 * S + 3) == S + 3
        # one entry is past what dfd_decoder_attn_fwd can merge (heads x splits floats of LDS): the GPU test sees it refused
        assert [s for s in sp if not dec.combine_fits(heads, s)] == ([3459] if (heads, S) == (16, 1728) else [])


def test_policy_splits_is_the_decoders():
    from dfd_clip_amd.decoder import Decoder
    for B in (1, 2, 3, 4, 16, 64):
        for S in (1, 15, 63, 64, 147, 1728, 5880, 16128):
            assert dec.policy_splits(B, S) == Decoder._splits(None, B, S)
    assert dec.policy_splits(1, 30 * 196) == 91


def test_rows_per_block_fits_a_workgroup():
    for heads in range(1, 17):
        R = dec.rows_per_block(heads)
        threads = heads * 8 * R
        assert R >= 1 and threads % 64 == 0 and 256 <= threads <= 1024, (heads, R, threads)
        assert R == 1 or heads * 8 * (R - 1) < 256 or (heads * 8 * (R - 1)) % 64 != 0, "R is the smallest such count"
