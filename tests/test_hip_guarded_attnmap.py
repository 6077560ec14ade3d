"""Guard-band and strided-view runs of the entry point of include/dfdclip_explain.h, with the harness of
tests/test_hip_guarded.py (tests/guarded.py): `aff` and `branches` between NaN-poisoned guards and NaN inside, K a strided
view of a q|k|v activation whose CLS rows and Q / V thirds are poisoned, `stats` and `ext_weights` of the exact size.
Asserted: no byte outside a view changed, no poison read, no element left unwritten, guarded = dense bit for bit.

Coverage (checked against include/dfdclip_explain.h by tests/test_attnmap_cpu.py):

    dfd_decoder_attn_map                  test_decoder_attn_map
"""
import pytest
import torch

from tests.attnmap_cases import attention_branches
from tests.test_hip_guarded import BF16, F32, both, capi, rnd, verify  # noqa: F401  (capi: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("modes", [0, 3])
@pytest.mark.parametrize("B,T,P,heads", [(1, 1, 1, 1), (9, 3, 101, 2), (2, 1, 257, 4), (64, 2, 7, 4)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decoder_attn_map(capi, B, T, P, heads, dtype, modes):
    """Rows of 1 ... 257 keys; clip 1 has a padded tail where the shape and the mode allow one."""
    D, S, tok = heads * 64, T * P, P + 1
    k = rnd(B, S, D, seed=1).to(dtype).float()
    q = rnd(B, heads, 128, seed=3)
    pos = 0.3 * rnd(T, D, seed=4)
    m = torch.ones(B, T, dtype=torch.bool)
    if B > 1 and modes == 0 and T > 1:  # "frame" groups of a padded frame are NaN, in the reference as well
        m[1, T - 1:] = False
    kk = (k.view(B, T, P, D) + pos.view(1, T, 1, D)).view(B, S, D)
    ws_, wc_ = attention_branches(q, kk, m, T, ("frame", "temporal") if modes else ())
    qkv = torch.full((B * T, tok, 3 * D), float("nan"))
    qkv[:, 1:, D:2 * D] = k.reshape(B * T, P, D)
    qkv = qkv.to(dtype).reshape(B * T * tok, 3 * D)
    # the forward's statistics / the grouped-softmax weights, made once on dense buffers: inputs of the call under test
    f32 = dict(device="cuda", dtype=torch.float32)
    qd0, md0 = q.reshape(B, 2 * D).cuda(), m.to(torch.uint8).cuda()
    kd0 = kk.cuda()
    stats0 = aw0 = None
    if modes:
        sc0, aw0 = torch.empty(B, heads, S, **f32), torch.empty(B, heads, S, **f32)
        capi.decoder_attn_modes_fwd(qd0, kd0, md0, modes, sc0, aw0, B, T, P, heads)
    else:
        ws0 = torch.empty(capi.decoder_attn_workspace_bytes(B, heads, 64, 3) // 4, **f32)
        mix0, stats0 = torch.empty(B, D, **f32), torch.empty(B, heads, 2, **f32)
        capi.decoder_attn_fwd(qd0, kd0, kd0, md0, mix0, stats0, ws0, 3, B, T, P, heads)

    def op(b):
        a2 = b.inp(qkv, pad=8, name="qkv")
        a3 = a2.as_strided((B * T, tok, 3 * D), (tok * a2.stride(0), a2.stride(0), 1))
        qd, md, pd = b.inp(q.reshape(B, 2 * D), name="q"), b.inp(m.to(torch.uint8), fill=1, name="frame_mask"), b.inp(pos, name="pos")
        st = b.inp(stats0.reshape(B, heads * 2).cpu(), name="stats") if stats0 is not None else None
        aw = b.inp(aw0.reshape(B * heads, S).cpu(), name="ext_weights") if aw0 is not None else None
        aff, br = b.out((B * heads, S), name="aff"), b.out((2 * B * heads, S), name="branches")
        capi.decoder_attn_map(qd, a3[:, 1:, D:2 * D], md, st, aff, B, T, P, heads, ext_weights=aw, branches=br, pos=pd)
        return {"aff": aff, "branches": br}
    verify(*both(op), {"aff": ((0.5 * (ws_ + wc_)).reshape(B * heads, S), 2e-5, 1e-4),
                       "branches": (torch.stack([ws_, wc_]).reshape(2 * B * heads, S), 2e-5, 1e-4)}, msg=f"attention map modes={modes}")
