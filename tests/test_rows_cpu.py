"""The row descriptor of the decode path without a GPU: which library entry point and workspace function each routing
combination names, what ``sub`` yields, and which combinations are refused.  CPU tensors stand in for the device tables."""
import pytest
import torch

from moondream_amd.moondream import _Rows


def table(n=6, base=0):
    return torch.arange(base, base + n, dtype=torch.int32)


class Bank:
    """Stand-in for a PackedLoraBank: the descriptor only carries it (and reads ``generation`` for graph keys)."""

    generation = 3


class Lora:
    """Stand-in for a PackedLora."""


SLOTS = dict(slots=table(), n_slots=12)
PREFIX = dict(prefix_slots=table(base=6), prefix_len=table(base=100))
VARIANTS = dict(variants=table(base=-1), bank=Bank())
# fields -> (forward, its workspace function, decode step, its workspace function), or ValueError
CASES = {
    "contiguous": (dict(slot0=2), ("md_text_forward", "md_text_workspace_bytes", "md_decode_step", "md_decode_workspace_bytes")),
    "int": (2, ("md_text_forward", "md_text_workspace_bytes", "md_decode_step", "md_decode_workspace_bytes")),
    "slot table": (SLOTS, ("md_text_forward_slots", "md_text_workspace_bytes", "md_decode_step_slots", "md_decode_workspace_bytes")),
    "prefix table": ({**SLOTS, **PREFIX},
                     ("md_text_forward_shared", "md_text_workspace_bytes", "md_decode_step_shared", "md_decode_workspace_bytes")),
    "variant table": ({"slot0": 2, **VARIANTS}, ("md_text_forward_multi_lora", "md_text_multi_lora_workspace_bytes",
                                                 "md_decode_step_multi_lora", "md_decode_multi_lora_workspace_bytes")),
    "variant + slot table": ({**SLOTS, **VARIANTS}, ("md_text_forward_multi_lora", "md_text_multi_lora_workspace_bytes",
                                                    "md_decode_step_multi_lora", "md_decode_multi_lora_workspace_bytes")),
    # a whole-call adapter has no fused step: the decode loop makes it from md_text_forward_lora and its pieces
    "PackedLora": (dict(slot0=2, lora=Lora()), ("md_text_forward_lora", "md_text_lora_workspace_bytes", None, None)),
    "prefix + variants": ({**SLOTS, **PREFIX, **VARIANTS}, ValueError),
    "prefix + PackedLora": ({**SLOTS, **PREFIX, "lora": Lora()}, ValueError),
    "variants + PackedLora": ({**VARIANTS, "lora": Lora()}, ValueError),
    "prefix without slot table": (PREFIX, ValueError),
    "half a prefix table": ({**SLOTS, "prefix_slots": table()}, ValueError),
    "variants without bank": (dict(variants=table()), ValueError),
    "slot table + PackedLora": ({**SLOTS, "lora": Lora()}, ValueError),
    "slot table + slot0": ({**SLOTS, "slot0": 1}, ValueError),
    "slot table without n_slots": (dict(slots=table()), ValueError),
}


@pytest.mark.parametrize("name", list(CASES))
def test_rows_name_their_entry_points_and_slice(name):
    fields, want = CASES[name]
    if want is ValueError:
        with pytest.raises(ValueError):
            _Rows(**fields)
        return
    rows = _Rows.of(fields) if isinstance(fields, int) else _Rows(**fields)
    assert _Rows.of(rows) is rows
    assert (rows.forward_entry, rows.forward_ws_entry, rows.step_entry, rows.step_ws_entry) == want
    assert rows.plain == (want[0] == "md_text_forward")
    fields = dict(slot0=fields) if isinstance(fields, int) else fields
    sub = rows.sub(1, 4)
    assert (sub.forward_entry, sub.step_entry) == want[::2]  # the same routing ...
    for f in ("slots", "prefix_slots", "prefix_len", "variants"):  # ... over rows 1 .. 3 of every table: views, no copies
        if fields.get(f) is None:
            assert getattr(sub, f) is None
        else:
            assert torch.equal(getattr(sub, f), fields[f][1:4]) and getattr(sub, f).data_ptr() == fields[f][1:4].data_ptr()
    assert sub.lora is rows.lora and sub.bank is rows.bank and sub.n_slots == rows.n_slots
    if "slots" in fields:
        assert sub.slot0 == 0 and rows.span(6) == sub.span(3) == 12  # a table addresses the whole slab
    else:
        assert sub.slot0 == 3 and rows.span(6) == 8 and sub.span(3) == 6
    # the graph key names exactly what a capture bakes in, and tells the rows of a table apart
    slots_key = (fields["slots"].data_ptr(), 12) if "slots" in fields else 2
    prefix_key = (fields["prefix_slots"].data_ptr(), fields["prefix_len"].data_ptr()) if "prefix_slots" in fields else None
    variants_key = (fields["variants"].data_ptr(), 3) if "variants" in fields else None
    assert rows.key() == (slots_key, prefix_key, variants_key)
    assert sub.key() != rows.key()
