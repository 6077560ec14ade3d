"""CPU side of the any-token-count encoder: the 577-token geometries exist (`ViT-L/14@336px` and the test model
`small24`), the CPU oracle reproduces the reference's own results on `small24` (tests/golden/small24.npz, written by
tools/gen_golden_anytok.py; the 2e-5 bar of tests/test_oracle_golden.py), the checkpoint loader reads a 336-px tower off
the tensor shapes, and the attention test hook is exported next to the ABI and keeps its value per thread."""
import threading

import numpy as np
import torch

from dfd_clip_amd.build import build
from dfd_clip_amd.weights import ARCHS, REFERENCE_CLIP_NAMES
from oracle import ref_cpu
from tests.anytok_cases import CASES, build_case, load_golden, oracle_kwargs
from tests.cases import synthetic_clip_checkpoint

TOL = 2e-5


def test_archs_have_the_577_token_geometries():
    assert ARCHS["ViT-L/14@336px"] == (336, 14, 1024, 24, 16, 768)
    assert ARCHS["small24"] == (336, 14, 128, 2, 2, 64)
    assert "ViT-L/14@336px" in REFERENCE_CLIP_NAMES
    for name in ("ViT-L/14@336px", "small24"):
        res, patch = ARCHS[name][:2]
        assert (res // patch) ** 2 + 1 == 577 and 3 * patch * patch == 588


def test_oracle_matches_reference_on_small24():
    assert list(CASES) == ["small24"]
    case = build_case("small24")
    g = load_golden("small24")
    with torch.no_grad():
        losses, logits = ref_cpu.detector_forward_eval(case["sd"], case["x"], [case["y"]], case["m"], single_task=0, **oracle_kwargs(case))
        _, feat = ref_cpu.detector_predict(case["sd"], case["x"], case["m"], **oracle_kwargs(case))
        kvs = ref_cpu.encoder_forward(case["sd"], case["x"].flatten(0, 1), case["heads"], case["patch"], with_out=True)
    np.testing.assert_allclose(logits[0].numpy(), g["logits"], atol=TOL, rtol=0)
    np.testing.assert_allclose(losses[0].numpy(), g["losses"], atol=TOL, rtol=1e-5)
    np.testing.assert_allclose(feat.numpy(), g["video_feature"], atol=TOL, rtol=0)
    assert list(g["layer_indices"]) == case["layer_indices"] == [0, 1]
    rows, n = list(g["slice_rows"]), case["B"] * case["T"]
    assert kvs[0]["k"].shape[1] == 577
    for l in case["layer_indices"]:
        for key in ("k", "v"):
            for fr in (0, n - 1):
                np.testing.assert_allclose(kvs[l][key][fr, rows].numpy(), g[f"enc{l}_{key}_f{fr}"], atol=TOL, rtol=0)
    for key in ("train_task_loss", "step_losses", "logits_bf16", "video_feature_bf16"):
        assert key in g.files, key
    assert np.abs(g["logits_bf16"] - g["logits"]).max() < 0.15


def test_loader_reads_a_336px_tower_off_the_shapes(tmp_path):
    from dfd_clip_amd.detector import load_clip_visual
    build()
    sd = synthetic_clip_checkpoint("small24", dtype=torch.float16)
    path = str(tmp_path / "ckpt336.pt")
    torch.save(sd, path)
    vit = load_clip_visual(path, "fp32")
    assert (vit.input_resolution, vit.patch_size, vit.width, vit.layers, vit.heads, vit.output_dim) == ARCHS["small24"]
    assert vit.state_dict()["positional_embedding"].shape == (577, 128)


def test_attention_variant_hook_is_exported_and_per_thread():
    from dfd_clip_amd import capi
    build()
    lib = capi.load_library()
    for name in ("dfd_attention_set_variant", "dfd_attention_last_path", "dfd_attention_plan"):
        assert name in capi.HOOK_SIGNATURES and name not in capi.SIGNATURES and hasattr(lib, name), name
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17
    assert capi.attention_set_variant(2) == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(capi.attention_set_variant(1)))
    t.start()
    t.join()
    assert seen == [0], "another thread starts at the default"
    # the plan hook answers under the calling thread's variant: here 2 (no streaming kernel), in a new thread the default
    paths = [capi.attention_plan(torch.bfloat16, 2, 50, 2).path]
    t = threading.Thread(target=lambda: paths.append(capi.attention_plan(torch.bfloat16, 2, 50, 2).path))
    t.start()
    t.join()
    assert paths == [capi.ATTN_ROWS, capi.ATTN_STREAM]
    assert capi.attention_set_variant(0) == 2 and capi.attention_set_variant(0) == 0
    # no attention call on this thread or a new one yet: the last path is per thread and starts at 0
    t = threading.Thread(target=lambda: seen.append(capi.attention_last_path()))
    t.start()
    t.join()
    assert seen == [0, 0]
