"""Mixed LoRA variants without a GPU: the bank's packing (ranks rounded to 16, missing pairs, the rank limit), the host-side
argument checks of the new entry points, the md_lora_bank layout against the header, and the argument checks of
batch_generate_ids(variants=...)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.weights import pack_lora_variant

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 1, 4


def test_pack_rounds_ranks_to_16_and_keeps_missing_pairs_missing():
    cfg = get_config("tiny")
    lora = synth.synthetic_lora(cfg, seed=3, rank=8)
    blocks = lora["text"]["blocks"]
    # mixed ranks: fc1 at rank 40 in layer 0 only, fc2 absent from layer 1
    f1 = blocks["0"]["mlp"]["fc1"]
    f1["A"] = torch.randn(40, cfg.text.dim).to(torch.bfloat16)
    f1["B"] = torch.randn(cfg.text.ff_dim, 40).to(torch.bfloat16)
    del blocks["1"]["mlp"]["fc2"]
    ranks, layers = pack_lora_variant(cfg, lora)
    assert ranks == [16, 16, 48, 16]
    assert layers[1][3] is None and layers[0][3] is not None
    a, b = layers[0][2]
    assert tuple(a.shape) == (48, cfg.text.dim) and tuple(b.shape) == (cfg.text.ff_dim, 48)
    assert torch.equal(a[:40], f1["A"]) and torch.equal(b[:, :40], f1["B"])
    assert not a[40:].any() and not b[:, 40:].any()
    # layer 1's fc1 (rank 8) is padded to the pair's packed rank, 48
    a1, b1 = layers[1][2]
    assert tuple(a1.shape) == (48, cfg.text.dim) and not a1[8:].any() and not b1[:, 8:].any()
    qa, qb = layers[2][0]
    assert tuple(qa.shape) == (16, cfg.text.dim) and tuple(qb.shape) == (cfg.text.qkv_dim, 16)


def test_pack_refuses_rank_above_256_and_bad_shapes():
    cfg = get_config("tiny")
    lora = synth.synthetic_lora(cfg, seed=1, rank=8)
    p = lora["text"]["blocks"]["2"]["attn"]["proj"]
    p["A"] = torch.zeros(272, cfg.text.dim, dtype=torch.bfloat16)
    p["B"] = torch.zeros(cfg.text.dim, 272, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="above 256"):
        pack_lora_variant(cfg, lora)
    lora = synth.synthetic_lora(cfg, seed=1, rank=8)
    lora["text"]["blocks"]["0"]["attn"]["qkv"]["B"] = torch.zeros(5, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        pack_lora_variant(cfg, lora)
    ranks, _ = pack_lora_variant(cfg, synth.synthetic_lora(cfg, seed=1, rank=256))
    assert ranks == [256] * 4


def test_multi_lora_entry_points_validate_on_the_host():
    lib = _lib.load()
    d = ctypes.c_void_p(0x10)  # never dereferenced: every call below fails its host checks first
    bank = _lib.MdLoraBank()
    assert lib.md_lora_bank_table_bytes(24) == 24 * 16 * 4 * 16
    assert lib.md_lora_bank_table_bytes(0) == 0
    assert lib.md_lora_bank_init(None, 24, d, 1 << 20) == ERR_ARG
    assert lib.md_lora_bank_init(ctypes.byref(bank), 24, None, 1 << 20) == ERR_ARG
    assert lib.md_lora_bank_init(ctypes.byref(bank), 24, d, 100) == ERR_ARG  # table too small
    m = _lib.MdTextModel()
    m.n_layers, m.n_heads, m.n_kv_heads, m.dim = 3, 4, 4, 256
    bank.n_layers, bank.table = 3, 0x1000
    assert lib.md_lora_bank_set_variant(ctypes.byref(bank), ctypes.byref(m), 17, d) == ERR_ARG  # beyond 16 variants
    assert lib.md_lora_bank_set_variant(ctypes.byref(bank), ctypes.byref(m), 1, d) == ERR_ARG   # a gap: only index 0 may come next
    assert lib.md_lora_bank_set_variant(ctypes.byref(bank), ctypes.byref(m), 0, None) == ERR_ARG
    # an empty bank, a bank with a rank that is no multiple of 16, a NULL table
    for n_var, rank, table in ((0, 16, 0x1000), (1, 24, 0x1000), (1, 16, None), (17, 16, 0x1000)):
        bank.n_variants, bank.table = n_var, table
        bank.rank[0][0] = rank
        assert lib.md_lora_shrink_grouped(ctypes.byref(bank), 0, 7, d, 4, 1, d, 256, 256, d, 256, None) == ERR_ARG
        assert lib.md_lora_expand_grouped(ctypes.byref(bank), 0, 0, 7, d, 4, 1, d, 256, d, 768, 768, 0, -1, None) == ERR_ARG
    bank.n_variants, bank.table, bank.rank[0][0] = 1, 0x1000, 16
    # bad shapes: layer out of range, k not a multiple of 32, NULL variant table, n not a multiple of 16, an unknown flag
    assert lib.md_lora_shrink_grouped(ctypes.byref(bank), 3, 7, d, 4, 1, d, 256, 256, d, 256, None) == ERR_ARG
    assert lib.md_lora_shrink_grouped(ctypes.byref(bank), 0, 7, d, 4, 1, d, 256, 200, d, 256, None) == ERR_ARG
    assert lib.md_lora_shrink_grouped(ctypes.byref(bank), 0, 7, None, 4, 1, d, 256, 256, d, 256, None) == ERR_ARG
    assert lib.md_lora_shrink_grouped(ctypes.byref(bank), 0, 7, d, 4, 1, d, 256, 256, d, 8, None) == ERR_ARG  # ldt < width
    assert lib.md_lora_expand_grouped(ctypes.byref(bank), 0, 0, 7, d, 4, 1, d, 256, d, 768, 760, 0, -1, None) == ERR_ARG
    assert lib.md_lora_expand_grouped(ctypes.byref(bank), 0, 0, 7, d, 4, 1, d, 256, d, 768, 768, 5, -1, None) == ERR_ARG
    assert lib.md_lora_expand_grouped(ctypes.byref(bank), 0, 3, 7, d, 4, 1, d, 256, d, 768, 768, 0, -1, None) == ERR_ARG  # pair not in t
    # the forward / decode entry points: NULL bank = the *_slots function (which rejects this empty model); the fp8 modes
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    assert lib.md_text_forward_multi_lora(ctypes.byref(m), None, None, d, d, 2, 1, d, None, 0, ctypes.byref(kv), d, 1 << 20,
                                          None) == ERR_ARG
    assert lib.md_decode_step_multi_lora(ctypes.byref(m), None, None, d, d, d, 2, None, 0, ctypes.byref(kv), 0, d, 64, d, 1 << 20,
                                         None) == ERR_ARG
    blocks = (_lib.MdTextBlock * 3)()
    m.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.MdTextBlock))
    assert lib.md_text_forward_multi_lora(ctypes.byref(m), ctypes.byref(bank), None, d, d, 2, 1, d, None, 0, ctypes.byref(kv), d,
                                          1 << 20, None) == ERR_ARG  # no variant table
    assert lib.md_text_forward_multi_lora(ctypes.byref(m), ctypes.byref(bank), d, d, d, 2, 1, d, d, 0, ctypes.byref(kv), d,
                                          1 << 20, None) == ERR_ARG  # a slot table with n_slots 0
    kv8 = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    kv8.k8, kv8.v8 = 0x3000, 0x4000
    assert lib.md_text_forward_multi_lora(ctypes.byref(m), ctypes.byref(bank), d, d, d, 2, 1, d, None, 0, ctypes.byref(kv8), d,
                                          1 << 20, None) == ERR_UNSUPPORTED
    assert lib.md_decode_step_multi_lora(ctypes.byref(m), ctypes.byref(bank), d, d, d, d, 2, None, 0, ctypes.byref(kv8), 0, d, 64,
                                         d, 1 << 20, None) == ERR_UNSUPPORTED
    base = lib.md_text_workspace_bytes(ctypes.byref(m), 2, 1)
    assert lib.md_text_multi_lora_workspace_bytes(ctypes.byref(m), None, 2, 1) == base


def test_lora_bank_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    header = os.path.join(REPO, "include", "moondream_hip.h")
    src = tmp_path / "bank.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {",
        '  printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(md_lora_bank), offsetof(md_lora_bank, n_variants),'
        " offsetof(md_lora_bank, n_layers), offsetof(md_lora_bank, rank), offsetof(md_lora_bank, table),"
        " MD_LORA_MAX_VARIANTS, MD_LORA_MAX_RANK);",
        '  printf("%d %d %d %d %d %d\\n", MD_LORA_QKV, MD_LORA_PROJ, MD_LORA_FC1, MD_LORA_FC2, MD_LORA_ADD, MD_LORA_DELTA);',
        "  return 0;", "}"]))
    exe = tmp_path / "bank"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    line1, line2 = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")[:2]
    size, o_nv, o_nl, o_rank, o_table, max_v, max_r = (int(v) for v in line1.split())
    B = _lib.MdLoraBank
    assert ctypes.sizeof(B) == size
    assert [B.n_variants.offset, B.n_layers.offset, B.rank.offset, B.table.offset] == [o_nv, o_nl, o_rank, o_table]
    assert (max_v, max_r) == (_lib.MD_LORA_MAX_VARIANTS, _lib.MD_LORA_MAX_RANK)
    assert [int(v) for v in line2.split()] == [_lib.MD_LORA_QKV, _lib.MD_LORA_PROJ, _lib.MD_LORA_FC1, _lib.MD_LORA_FC2,
                                               _lib.MD_LORA_ADD, _lib.MD_LORA_DELTA]


def test_batch_generate_ids_checks_variants_before_any_gpu_work():
    from moondream_amd.moondream import MoondreamModel

    model = MoondreamModel.__new__(MoondreamModel)  # no weights, no device: the checks come first
    with pytest.raises(ValueError, match="cannot be combined"):
        model.batch_generate_ids([None, None], [[1], [1]], variant="a", variants=["a", None])
    with pytest.raises(ValueError, match="entries"):
        model.batch_generate_ids([None, None], [[1], [1]], variants=["a"])


def test_engine_submit_resolves_variants_before_any_gpu_work():
    from types import SimpleNamespace

    from PIL import Image

    from moondream_amd.continuous import ContinuousEngine

    def resolve(vid):
        if vid == "known":
            return 3
        raise FileNotFoundError(vid)

    img = Image.new("RGB", (32, 32))
    eng = ContinuousEngine(SimpleNamespace(config=get_config("tiny"), _bank_index=resolve), max_live=2)
    with pytest.raises(ValueError, match="unknown LoRA variant"):
        eng.submit(img, [5], variant="unknown")
    eng.submit(img, [5], variant="known")
    eng.submit(img, [5])
    assert [r.variant for r in eng.sched.queue] == [3, -1]
    eng2 = ContinuousEngine(SimpleNamespace(config=get_config("tiny")), max_live=2)  # a model without variants
    with pytest.raises(ValueError):
        eng2.submit(img, [5], variant="known")


def test_registered_variants_are_kept_on_the_host():
    from moondream_amd.moondream import _tree_to_cpu

    cfg = get_config("tiny")
    lora = synth.synthetic_lora(cfg, seed=2, rank=8)
    cp = _tree_to_cpu(lora)
    a = lora["text"]["blocks"]["0"]["attn"]["qkv"]["A"]
    b = cp["text"]["blocks"]["0"]["attn"]["qkv"]["A"]
    assert b.device.type == "cpu" and torch.equal(a, b) and b.data_ptr() != a.data_ptr()
