"""Batched reasoning queries without a GPU: the host checks of md_decode_step_reason / md_reason_route /
md_mask_logits_rows (every refusal comes before any launch), the layout of the two new argument structs against the
header, the refusals of ``batch_query(..., reasoning=True)`` on a stub model, and the chunk runner's reasoning branch."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest

from moondream_amd import _lib
from moondream_amd.config import TokenizerConfig, get_config
from moondream_amd.decode_loop import DecodeChunk, ReasonChunk, Sampling, run_chunk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 1, 3, 4
D = ctypes.c_void_p(0x100)  # never dereferenced: every call below fails its host checks first


def lin(n, k):
    pad = lambda x: (x + 63) // 64 * 64
    return _lib.MdLinear(0x1000, 0x2000, n, k, pad(n), pad(k))


def tiny_text_model():
    """The tiny decoder's shapes over fake device pointers: enough for the workspace functions, never launched."""
    m = _lib.MdTextModel()
    m.n_layers, m.n_heads, m.n_kv_heads, m.dim, m.vocab, m.ff_dim = 3, 4, 4, 256, 1024, 704
    blocks = (_lib.MdTextBlock * 3)()
    for b in blocks:
        b.qkv, b.proj, b.fc1, b.fc2 = lin(768, 256), lin(256, 256), lin(704, 256), lin(256, 704)
    m.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.MdTextBlock))
    m.lm_head = lin(1024, 256)
    m.wte = 0x3000
    return m, blocks


def region_coord():
    return _lib.MdRegionCoord(lin(512, 256), lin(1024, 512), lin(256, 256), 0x4000, 0x5000, 128, 1024)


def reason_state(**kw):
    st = _lib.MdReasonState(0x100, 0x100, 0x100, 0x100, 0x100, 0x100, 0x100, 0x100, None, 8, 8, 3, 0, 6, 5, 3)
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_decode_step_reason_refuses_on_the_host():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    rc, kv = region_coord(), _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    need = lib.md_decode_reason_workspace_bytes(ctypes.byref(m), ctypes.byref(rc), 4)
    assert need > lib.md_decode_workspace_bytes(ctypes.byref(m), 4) > 0
    assert lib.md_decode_reason_workspace_bytes(None, ctypes.byref(rc), 4) == 0
    assert lib.md_decode_reason_workspace_bytes(ctypes.byref(m), None, 4) == 0
    assert lib.md_decode_reason_workspace_bytes(ctypes.byref(m), ctypes.byref(rc), 0) == 0

    def step(m=m, rc=rc, st=None, bank=None, tokens=D, pos=D, batch=4, slots=None, n_slots=0, pfx=None, plen=None, kv=kv, logits=D,
             ld=1024, ws=D, ws_bytes=need):
        st = st if st is not None else reason_state()
        ref = lambda s: ctypes.byref(s) if s is not None else None
        return lib.md_decode_step_reason(ref(m), ref(rc), ref(st), ref(bank), tokens, pos, batch, slots, n_slots, pfx, plen, ref(kv),
                                         logits, ld, ws, ws_bytes, None)

    # NULL arguments
    for name in ("m", "rc", "tokens", "pos", "kv", "logits", "ws"):
        assert step(**{name: None}) == ERR_ARG, name
    assert lib.md_decode_step_reason(ctypes.byref(m), ctypes.byref(rc), None, None, D, D, 4, None, 0, None, None, ctypes.byref(kv), D,
                                     1024, D, need, None) == ERR_ARG
    for field in ("phase", "n_reason", "n_answer", "kind", "ground", "suppress", "coord_bin", "hidden_prev"):
        assert step(st=reason_state(**{field: None})) == ERR_ARG, field
    # negative / out-of-range arguments
    assert step(batch=0) == ERR_ARG and step(batch=-1) == ERR_ARG
    assert step(st=reason_state(max_reason=-1)) == ERR_ARG and step(st=reason_state(max_answer=-1)) == ERR_ARG
    assert step(st=reason_state(suffix_id=-1)) == ERR_ARG and step(st=reason_state(suffix_id=1024)) == ERR_ARG
    assert step(ld=1023) == ERR_ARG
    assert step(slots=D, n_slots=0) == ERR_ARG             # a slot table with n_slots 0
    assert step(pfx=D, plen=D) == ERR_ARG                  # a prefix table without a slot table
    assert step(slots=D, n_slots=4, pfx=D) == ERR_ARG      # ... without its lengths
    # a region head that does not chain onto the model
    for field, bad in (("dec_fc1", lin(512, 320)), ("dec_fc2", lin(1024, 448)), ("dec_fc2", lin(1000, 512)), ("encoder", lin(256, 128)),
                       ("encoder", lin(320, 256))):
        rc2 = region_coord()
        setattr(rc2, field, bad)
        assert step(rc=rc2) == ERR_UNSUPPORTED, (field, bad.n, bad.k)
    rc2 = region_coord()
    rc2.half = 0
    assert step(rc=rc2) == ERR_ARG
    # the multi-LoRA bank is not served -- whatever the workspace
    bank = _lib.MdLoraBank()
    bank.n_layers, bank.n_variants, bank.table = 3, 1, 0x1000
    assert step(bank=bank) == ERR_UNSUPPORTED and step(bank=bank, ws_bytes=0) == ERR_UNSUPPORTED
    # a workspace one byte short
    assert step(ws_bytes=need - 1) == ERR_WORKSPACE and step(ws_bytes=0) == ERR_WORKSPACE


def test_route_and_mask_kernels_refuse_on_the_host():
    lib = _lib.load()

    def route(st=None, tokens=D, wte=D, ld_wte=256, vocab=1024, emb=D, ld_emb=256, x=D, ldx=256, batch=3, dim=256):
        st = st if st is not None else reason_state()
        return lib.md_reason_route(ctypes.byref(st), tokens, wte, ld_wte, vocab, emb, ld_emb, x, ldx, batch, dim, None)

    assert lib.md_reason_route(None, D, D, 256, 1024, D, 256, D, 256, 3, 256, None) == ERR_ARG
    for name in ("tokens", "wte", "emb", "x"):
        assert route(**{name: None}) == ERR_ARG, name
    for field in ("phase", "n_reason", "n_answer", "kind", "ground", "suppress", "coord_bin"):
        assert route(st=reason_state(**{field: None})) == ERR_ARG, field
    assert route(batch=0) == ERR_ARG and route(vocab=0) == ERR_ARG and route(dim=0) == ERR_ARG and route(dim=252) == ERR_ARG
    assert route(ld_wte=248) == ERR_ARG and route(ld_emb=248) == ERR_ARG and route(ldx=248) == ERR_ARG and route(ld_wte=260) == ERR_ARG
    assert route(wte=ctypes.c_void_p(0x108)) == ERR_ARG     # not 16-byte aligned
    assert route(st=reason_state(max_reason=-1)) == ERR_ARG and route(st=reason_state(suffix_id=1024)) == ERR_ARG
    assert lib.md_mask_logits_rows(None, 1024, 2, 1024, D, None) == ERR_ARG
    assert lib.md_mask_logits_rows(D, 1024, 2, 1024, None, None) == ERR_ARG
    assert lib.md_mask_logits_rows(D, 1024, 0, 1024, D, None) == ERR_ARG
    assert lib.md_mask_logits_rows(D, 1024, 2, 0, D, None) == ERR_ARG
    assert lib.md_mask_logits_rows(D, 1023, 2, 1024, D, None) == ERR_ARG


def test_reason_struct_layouts_match_the_header(tmp_path):
    """md_region_coord and md_reason_state against their ctypes mirrors: size and every field's offset as gcc lays the
    header out (the method of tests/test_abi.py::test_struct_layouts_match_the_header)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = {"md_region_coord": _lib.MdRegionCoord, "md_reason_state": _lib.MdReasonState}
    header = os.path.join(REPO, "include", "moondream_hip.h")
    text = open(header).read()
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {"]
    fields = {}
    for name in pairs:
        m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", text, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *rest = decl.split(",")
            names.append(first.split()[-1].lstrip("*"))
            names += [r.strip().lstrip("*") for r in rest]
        fields[name] = names
        lines.append(f'  printf("{name} %zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f in names]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(pairs)
    for line in out:
        name, size, *offs = line.split()
        cls = pairs[name]
        assert ctypes.sizeof(cls) == int(size), (name, ctypes.sizeof(cls), size)
        cnames = [f[0] for f in cls._fields_]
        assert cnames == fields[name], (name, cnames, fields[name])
        assert [getattr(cls, f).offset for f in cnames] == [int(o) for o in offs], name
    assert (_lib.MD_REASON_PHASE_IDLE, _lib.MD_REASON_PHASE_REASON, _lib.MD_REASON_PHASE_ANSWER, _lib.MD_REASON_PHASE_DONE) == (-1, 0, 1, 2)
    for name, val in (("MD_REASON_KIND_NONE", 0), ("MD_REASON_KIND_REASON", 1), ("MD_REASON_KIND_SUFFIX", 2), ("MD_REASON_KIND_ANSWER", 3)):
        assert re.search(name + r" = " + str(val) + r"\b", text) and getattr(_lib, name) == val


# ---------------------------------------------------------------- refusals of the public interface, on a stub
def stub_model(cfg=None, region=True, fp8=False, f8=False, kv8=False):
    from moondream_amd.moondream import MoondreamModel

    model = MoondreamModel.__new__(MoondreamModel)
    model.config = cfg or get_config("tiny")
    text = types.SimpleNamespace(fp8=object() if fp8 else None, f8=object() if f8 else None)
    model.w = types.SimpleNamespace(text=text, region={"coord_encoder": None} if region else None)
    model._kv8_scales = (1, 1) if kv8 else None
    return model


def test_reasoning_refusals_name_their_reason():
    imgs, qs = [object()], ["1 2"]
    for st in ({"variant": "v"}, {"variants": ["v"]}):
        with pytest.raises(NotImplementedError, match="LoRA"):
            stub_model().batch_query(imgs, qs, settings=st, reasoning=True)
        with pytest.raises(NotImplementedError, match="LoRA"):
            stub_model().query_many_reasoning(imgs[0], qs, settings=st)
    for kw in ({"fp8": True}, {"f8": True}, {"kv8": True}):
        with pytest.raises(NotImplementedError, match="fp8"):
            stub_model(**kw).batch_query(imgs, qs, reasoning=True)
        with pytest.raises(NotImplementedError, match="fp8"):
            stub_model(**kw).query_many_reasoning(imgs[0], qs)
    cfg = get_config("tiny")
    tpl = dict(cfg.tokenizer.templates)
    tpl["query"] = {"prefix": [1, 381, 2], "suffix": [3, 3]}
    two = type(cfg)(text=cfg.text, vision=cfg.vision, region=cfg.region, tokenizer=TokenizerConfig(templates=tpl))
    with pytest.raises(NotImplementedError, match="one-token query suffix"):
        stub_model(two).batch_query(imgs, qs, reasoning=True)
    with pytest.raises(NotImplementedError, match="region head"):
        stub_model(region=False).batch_query(imgs, qs, reasoning=True)
    with pytest.raises(NotImplementedError, match="region head"):
        stub_model(region=False).query_many_reasoning(imgs[0], qs)


def test_batch_query_without_reasoning_is_the_old_call():
    """reasoning=False: the same call into the generation route as before (``_generate_ids``, with the settings' record) and a
    list of strings back."""
    model = stub_model()
    seen = {}

    def fake_ids(images, prompts, st, **kw):
        seen["prompts"], seen["st"], seen["kw"] = prompts, st, kw
        return [[11, 12], [13]]

    model._generate_ids = fake_ids
    model.tokenizer = types.SimpleNamespace(encode=lambda q: types.SimpleNamespace(ids=[int(t) for t in q.split()]),
                                            decode=lambda ids: " ".join(str(i) for i in ids))
    for kw in ({}, {"reasoning": False}):
        out = model.batch_query([object(), object()], ["5 6", "7"], settings={"temperature": 0}, **kw)
        assert out == ["11 12", "13"] and all(isinstance(s, str) for s in out)
        assert seen["prompts"] == [[1, 381, 2, 5, 6, 3, 3], [1, 381, 2, 7, 3, 3]]  # suffix twice: no thinking token
        assert seen["st"].temperature == 0 and len(seen["st"].rows) == 2 and "reasoning" not in seen["kw"]


# ---------------------------------------------------------------- the chunk runner's reasoning branch
class Buf:
    def __init__(self, addr, rows=0):
        self.addr, self.rows = addr, rows

    def data_ptr(self):
        return self.addr

    def __getitem__(self, i):
        return Buf(self.addr + 64 * (i if isinstance(i, int) else 0))


class RecordingModel:
    """Stands in for the model: records the launches a chunk makes and the graph keys it asks for."""

    def __init__(self):
        self.calls, self.keys = [], []

    def _decode_logits(self, b):
        return Buf(0x9000)

    def _workspace(self, nbytes, which):
        return Buf(0xA000)

    def _kv_struct(self, slot0):
        return types.SimpleNamespace(k=0xB000, k8=None)

    def _decode_step(self, *a):
        self.calls.append(("step",))

    def _decode_step_reason(self, rows, reason, i, tok_in, pos, b, logits, ws, kv):
        self.calls.append(("reason_step", i, tok_in.data_ptr(), reason.kind[i].data_ptr()))

    def _pick_rows(self, logits, temperature, top_p, suppress_id, uniforms, out=None):
        self.calls.append(("pick_rows", suppress_id, uniforms.data_ptr(), out.data_ptr()))

    def _pick(self, *a, **k):
        self.calls.append(("pick",))

    def _token_logprobs(self, *a):
        self.calls.append(("logprobs",))

    def _replay_or_capture(self, key, body, may_capture=None):
        self.keys.append(key)
        body()
        return True


def reason_chunk(forced=None, base=0x100000):
    region = types.SimpleNamespace(dec_fc1=types.SimpleNamespace(w=0x77))
    bufs = [Buf(base + 0x1000 * j) for j in range(8)]
    return ReasonChunk(*bufs, 8, 8, region, forced)


def test_run_chunk_reason_branch_launches_and_keys():
    rows = types.SimpleNamespace(slot0=0, key=lambda: ("rows",))
    pick = Sampling(Buf(0x500), Buf(0x600))
    base = DecodeChunk(4, Buf(0x1000), Buf(0x2000), lambda i: rows, -1, 1 << 20, pick, Buf(0x3000))
    plain = RecordingModel()
    run_chunk(plain, base, 2, capture_stream=7)
    assert [c[0] for c in plain.calls] == ["step", "pick_rows", "step", "pick_rows"]  # unset: today's launches
    m = RecordingModel()
    chunk = DecodeChunk(4, Buf(0x1000), Buf(0x2000), lambda i: rows, -1, 1 << 20, pick, Buf(0x3000), reason=reason_chunk())
    run_chunk(m, chunk, 2, tag="reason", capture_stream=7)
    # every step: the fused reasoning step, then the per-row pick with nothing suppressed
    assert [c[0] for c in m.calls] == ["reason_step", "pick_rows", "reason_step", "pick_rows"]
    assert all(c[1] == -1 for c in m.calls if c[0] == "pick_rows")
    assert [c[1] for c in m.calls if c[0] == "reason_step"] == [0, 1]
    # the key: today's key for the same chunk, extended by the state's addresses
    same = RecordingModel()
    run_chunk(same, base, 2, tag="reason", capture_stream=7)
    assert m.keys[0][: len(same.keys[0])] == same.keys[0] and m.keys[0][len(same.keys[0])] == "reason"
    other = RecordingModel()
    run_chunk(other, DecodeChunk(4, Buf(0x1000), Buf(0x2000), lambda i: rows, -1, 1 << 20, pick, Buf(0x3000),
                                 reason=reason_chunk(base=0x200000)), 2, tag="reason", capture_stream=7)
    forced = RecordingModel()
    run_chunk(forced, DecodeChunk(4, Buf(0x1000), Buf(0x2000), lambda i: rows, -1, 1 << 20, pick, Buf(0x3000),
                                  reason=reason_chunk(forced=Buf(0x8000))), 2, tag="reason", capture_stream=7)
    assert len({m.keys[0], other.keys[0], forced.keys[0]}) == 3
    # eager: no key asked for
    eager = RecordingModel()
    run_chunk(eager, chunk, 1)
    assert eager.keys == [] and [c[0] for c in eager.calls] == ["reason_step", "pick_rows"]
    # a reasoning chunk always picks per row
    with pytest.raises(AssertionError):
        run_chunk(RecordingModel(), DecodeChunk(4, Buf(0x1000), Buf(0x2000), lambda i: rows, -1, 1 << 20, None, None,
                                                reason=reason_chunk()), 1)
