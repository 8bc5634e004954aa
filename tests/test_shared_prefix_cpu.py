"""Shared image prefix without a GPU: host-side argument validation of the shared-prefix entry points and the host planning
of the shared mode (rows -> prefix slots / own slots / prefill groups)."""
import ctypes

import pytest

from moondream_amd import _lib
from moondream_amd.config import get_config
from moondream_amd.shared_prefix import check_shared_table, plan_rows, plan_shared_prefix

ERR_ARG = 1


def kv_struct(k8=False):
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    if k8:
        kv.k8, kv.v8 = 0x3000, 0x4000
    return kv


def test_shared_entry_points_validate_on_the_host():
    lib = _lib.load()
    m = _lib.MdTextModel()
    d = ctypes.c_void_p(0x10)  # never dereferenced: every call below fails its host checks first
    kv, kv8 = kv_struct(), kv_struct(k8=True)
    for kvp in (None, ctypes.byref(kv8)):  # a NULL kv; the e4m3 copy of the fp8 mode
        assert lib.md_text_forward_shared(ctypes.byref(m), d, d, 2, 1, d, d, 4, d, d, kvp, d, 1 << 20, None) == ERR_ARG
        assert lib.md_decode_step_shared(ctypes.byref(m), d, d, d, 2, d, 4, d, d, kvp, 0, d, 64, d, 1 << 20, None) == ERR_ARG
    for n_slots in (0, -3):
        assert lib.md_text_forward_shared(ctypes.byref(m), d, d, 2, 1, d, d, n_slots, d, d, ctypes.byref(kv), d, 1 << 20,
                                          None) == ERR_ARG
        assert lib.md_decode_step_shared(ctypes.byref(m), d, d, d, 2, d, n_slots, d, d, ctypes.byref(kv), 0, d, 64, d, 1 << 20,
                                         None) == ERR_ARG
        assert lib.md_attention_decode_shared(d, 64, d, 64, d, d, 64, 16, d, 2, 1, 1, 64, 0.125, d, n_slots, d, d, None) == ERR_ARG
        assert lib.md_attention_decode_rope_shared(d, 192, d, 64, d, d, d, 64, 16, d, 2, 1, 64, 32, 0.125, d, n_slots, d, d,
                                                   None) == ERR_ARG
    # a prefix table needs the slot table and the prefix lengths
    assert lib.md_text_forward_shared(ctypes.byref(m), d, d, 2, 1, d, None, 4, d, d, ctypes.byref(kv), d, 1 << 20, None) == ERR_ARG
    assert lib.md_decode_step_shared(ctypes.byref(m), d, d, d, 2, d, 4, d, None, ctypes.byref(kv), 0, d, 64, d, 1 << 20,
                                     None) == ERR_ARG
    assert lib.md_attention_decode_shared(d, 64, d, 64, d, d, 64, 16, d, 2, 1, 1, 64, 0.125, None, 4, d, d, None) == ERR_ARG
    # kernel level: shape checks of the grouped kernel (head_dim 64, a context within the score buffer, FUSED is MHA)
    assert lib.md_attention_decode_shared(d, 64, d, 64, d, d, 64, 16, d, 2, 1, 1, 72, 0.125, d, 4, d, d, None) == ERR_ARG
    assert lib.md_attention_decode_shared(d, 64, d, 64, d, d, 64, 4096, d, 2, 1, 1, 64, 0.125, d, 4, d, d, None) == ERR_ARG
    assert lib.md_attention_decode_shared(d, 192, d, 192, d, d, 64, 16, d, 2, 3, 2, 64, 0.125, d, 4, d, d, None) == ERR_ARG


class Img:
    """An image stand-in: the planner only uses identity."""


def test_plan_dedups_by_identity_and_keeps_image_rows_contiguous_per_length():
    a, b, c = Img(), Img(), Img()
    images = [a, b, a, c, b, a, a, c]
    lens = [5, 5, 3, 5, 3, 5, 3, 5]
    plan = plan_shared_prefix(images, lens)
    assert plan.distinct == [a, b, c]  # first appearance; same object -> one prefix slot
    assert plan.n_slots == 3 + 8
    assert plan.own_slots == list(range(3, 11))
    assert sorted(plan.order) == list(range(8))
    # groups: one per prompt length, ascending
    assert plan.groups == [(0, 3), (3, 8)]
    for r0, r1 in plan.groups:
        assert len({lens[plan.order[r]] for r in range(r0, r1)}) == 1
        # each image's rows contiguous inside the group, callers ascending within an image
        ks = plan.prefix_slots[r0:r1]
        assert ks == sorted(ks)
        for k in set(ks):
            callers = [plan.order[r] for r in range(r0, r1) if plan.prefix_slots[r] == k]
            assert callers == sorted(callers)
    for r, src in enumerate(plan.order):
        assert plan.distinct[plan.prefix_slots[r]] is images[src]
    # mapping back to caller order and to the copy path's row order (stable sort by prompt length)
    copy_order = sorted(range(8), key=lambda i: lens[i])
    for r, src in enumerate(plan.order):
        assert copy_order[plan.copy_rank[r]] == src


def test_plan_mixed_raw_and_encoded_images():
    class Enc:
        pass

    raw, enc = Img(), Enc()
    other_raw = Img()
    plan = plan_shared_prefix([enc, raw, raw, enc, other_raw], [4, 4, 4, 4, 4])
    assert plan.distinct == [enc, raw, other_raw]
    assert plan.prefix_slots == [0, 0, 1, 1, 2]
    assert plan.order == [0, 3, 1, 2, 4]
    # equal but distinct objects are NOT merged
    x, y = Img(), Img()
    assert len(plan_shared_prefix([x, y], [1, 1]).distinct) == 2


def test_plan_rejects_bad_input():
    with pytest.raises(ValueError):
        plan_shared_prefix([], [])
    with pytest.raises(ValueError):
        plan_shared_prefix([Img()], [1, 2])


def test_shared_table_contract_checks():
    ok = dict(own_slots=[3, 4, 5], prefix_slots=[0, 0, 2], prefix_len=[730, 730, 730], pos0=[730, 735, 740], n_slots=6)
    check_shared_table(**ok)
    check_shared_table(**{**ok, "prefix_slots": [-1, 0, 2], "pos0": [0, 730, 730]})  # no prefix: any position
    bad = [
        {"pos0": [729, 730, 730]},            # writes inside its shared prefix
        {"prefix_slots": [0, 4, 2]},          # a prefix slot that is another row's own slot
        {"own_slots": [3, 3, 5]},             # two rows write one slot
        {"own_slots": [3, 4, 6]},             # own slot out of range
        {"prefix_slots": [0, 0, 7]},          # prefix slot out of range
        {"prefix_len": [730, 730]},           # tables of different lengths
    ]
    for b in bad:
        with pytest.raises(ValueError):
            check_shared_table(**{**ok, **b})


def test_share_prefix_defaults_off():
    import inspect

    from moondream_amd.moondream import MoondreamModel

    assert inspect.signature(MoondreamModel.batch_generate_ids).parameters["share_prefix"].default is False
    for name in ("query_many", "detect_many", "point_many"):
        assert list(inspect.signature(getattr(MoondreamModel, name)).parameters)[1:] == ["image", "questions" if name == "query_many" else "objects", "settings"]
    assert get_config("tiny").text.n_heads % get_config("tiny").text.n_kv_heads == 0


# ------------------------------------------------------------------ one plan for both routings (plan_rows)
def test_copy_plan_is_the_stable_sort_by_length_with_every_row_its_own_image():
    a, b = Img(), Img()
    images = [a, b, a, a, b, Img()]  # repeated objects: the copy path places each row's own
    lens = [5, 3, 5, 3, 4, 3]
    plan = plan_rows(images, lens, share=False)
    assert plan.order == sorted(range(6), key=lambda i: lens[i]) == [1, 3, 5, 4, 0, 2]
    assert len(plan.placed) == 6 and all(plan.placed[r] is images[plan.order[r]] for r in range(6))  # image r -> slot r
    assert plan.own_slots == list(range(6)) and plan.n_slots == 6
    assert plan.prefix_slots == []  # no prefix table
    assert plan.groups == [(0, 3), (3, 4), (4, 6)]
    assert plan.copy_rank == list(range(6))
    with pytest.raises(ValueError):
        plan_rows([], [], share=False)
    with pytest.raises(ValueError):
        plan_rows([a], [1, 2], share=False)


def shared_cases():
    a, b, c = Img(), Img(), Img()
    return [([a, b, a, c, b, a, a, c], [5, 5, 3, 5, 3, 5, 3, 5]), ([a, b, b, a, c], [4, 4, 4, 4, 4]), ([a, b], [1, 1])]


FIELDS = ("placed", "distinct", "order", "own_slots", "prefix_slots", "groups", "copy_rank", "n_slots")


def test_shared_plan_is_plan_shared_prefix():
    for images, lens in shared_cases():
        got, want = plan_rows(images, lens, share=True), plan_shared_prefix(images, lens)
        for f in FIELDS:
            assert getattr(got, f) == getattr(want, f), f
        p = len(want.distinct)
        assert want.n_slots == p + len(images) and want.own_slots == [p + r for r in range(len(images))]


def test_copy_rank_is_the_row_of_the_same_caller_in_the_copy_plan():
    for images, lens in shared_cases():
        shared, copy = plan_rows(images, lens, share=True), plan_rows(images, lens, share=False)
        for r, src in enumerate(shared.order):
            assert copy.order[shared.copy_rank[r]] == src


def test_prepared_in_caller_order_inverts_the_plan_order():
    from moondream_amd.moondream import Prepared

    images, lens = shared_cases()[0]
    variants = [3, -1, 0, 2, -1, 1, 0, 3]  # per row, in the caller's order
    for share in (False, True):
        plan = plan_rows(images, lens, share)
        per_slot = [f"row of caller {src}" for src in plan.order]
        prep = Prepared(order=plan.order, first=per_slot, hidden_last=per_slot, next_pos=[730 + lens[i] for i in plan.order],
                        rows=None, sampling=None)
        assert prep.in_caller_order(per_slot) == [f"row of caller {i}" for i in range(8)]
        # the variant table goes through the same ``order`` into slot order, and back
        table = [variants[i] for i in plan.order]
        assert all(table[r] == variants[src] for r, src in enumerate(plan.order))
        assert prep.in_caller_order(table) == variants
        assert prep.pos == prep.next_pos  # two prompt lengths: one position per row
    one = Prepared(order=[0, 1], first=None, hidden_last=None, next_pos=[735, 735], rows=None, sampling=None)
    assert one.pos == 735
