"""MoondreamModel: the reference's Python API on top of libmoondream_hip.so.

Public surface mirrors the reference class (reference:
moondream/torch/moondream.py:81-973): ``encode_image``, ``caption``, ``query``,
``detect``, ``point``, ``load_encoded_image``, ``compile`` and the four seam
methods ``_vis_enc / _vis_proj / _prefill / _decode_one_tok``
(moondream.py:168-192) -- here bound to hand-written gfx950 kernels through the
C ABI instead of ATen ops.  New: ``batch_generate`` / ``batch_caption`` /
``batch_query`` run B images in lockstep (the reference has no batching;
hf_moondream.py:99-103 is a sequential loop) and return what the sequential
path returns (bit for bit under ``set_strict_batch_invariance``; see
``batch_generate_ids`` for the default mode's contract).

PyTorch is used for device memory, streams and (optionally) hipGraph capture
only.  There is no eager / CPU fallback: without the built library or a GPU the
constructor raises.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import dataclass, replace
from functools import partial
from typing import Any, Dict, Iterable, List, Literal, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image

from . import _lib, grammar, resample
from . import stop as stops
from .config import MoondreamConfig
from .constraint import FREE, TokenAutomaton, check_constraints, pack, pow2_at_least
from .crop_staging import CropStager, crop_workers, plan_chunks, upload_unique
from .beam import Hypothesis, check_beams, finalize, inv_norm_table
from .decode_loop import (Beam, Constraint, DecodeChunk, Penalty, ReasonChunk, Sampling, Stop, check_score_settings,
                          check_top_logprobs, pick_tokens, run_chunk)
from .graph_store import GraphStore
from .image_crops import crop_count, overlap_crop_image, reconstruct_from_crops, resize_backend
from .integration import MASK_CAUSAL, MASK_PREFIX_LM, classify_attn_mask
from .lora import variant_state_dict
from .scores import Scores
from .settings import DEFAULT_MAX_TOKENS, DEFAULT_TEMPERATURE, DEFAULT_TOP_P, FAMILIES, CallSettings, refuse_settings
from .shared_prefix import RowPlan, check_shared_table, plan_rows
from .spatial import SpatialRecord, check_spatial_refs, refs_of, spatial_prompt_ids
from .weights import PackedLora, PackedLoraBank, PackedModel

BF16 = torch.bfloat16

DEFAULT_MAX_OBJECTS = 50

SpatialRefs = List[Union[Tuple[float, float], Tuple[float, float, float, float]]]


@dataclass(frozen=True)
class EncodedImage:
    """reference: moondream.py:56-59."""

    pos: int
    caches: List[Tuple[torch.Tensor, torch.Tensor]]


@dataclass(frozen=True, eq=False)
class _Rows:
    """How the B rows of a decoder call are routed: which KV slots they live in and which adapters they carry.  Slots:
    contiguous from ``slot0``, or ``slots`` (device int32 [B]; -1: an idle row) over ``n_slots`` slab slots.  With
    ``prefix_slots`` / ``prefix_len`` (device int32 [B]) row b reads its first prefix_len[b] positions from slot
    prefix_slots[b].  ``variants`` (device int32 [B], -1: the base model) gives each row a LoRA variant of ``bank``;
    ``lora`` is one adapter for the whole call.  Which fields are set decides the library entry point, its workspace
    function and what a captured graph bakes in -- here, in one place.  Combinations the library does not serve raise
    ValueError.  An int where a ``_Rows`` is expected means contiguous from that slot (``of``)."""

    slot0: int = 0
    slots: Optional[torch.Tensor] = None
    n_slots: int = 0
    prefix_slots: Optional[torch.Tensor] = None
    prefix_len: Optional[torch.Tensor] = None
    variants: Optional[torch.Tensor] = None
    bank: Optional[PackedLoraBank] = None
    lora: Optional[PackedLora] = None

    #         kind: (forward, its workspace function, decode step, its workspace function)
    _ENTRY = {
        "": ("md_text_forward", "md_text_workspace_bytes", "md_decode_step", "md_decode_workspace_bytes"),
        "_slots": ("md_text_forward_slots", "md_text_workspace_bytes", "md_decode_step_slots", "md_decode_workspace_bytes"),
        "_shared": ("md_text_forward_shared", "md_text_workspace_bytes", "md_decode_step_shared", "md_decode_workspace_bytes"),
        "_multi_lora": ("md_text_forward_multi_lora", "md_text_multi_lora_workspace_bytes", "md_decode_step_multi_lora",
                        "md_decode_multi_lora_workspace_bytes"),
        # the fused device-resident step has no single-adapter side path: the decode loop makes the step from its pieces
        "_lora": ("md_text_forward_lora", "md_text_lora_workspace_bytes", None, None),
    }

    def __post_init__(self):
        prefix = self.prefix_slots is not None or self.prefix_len is not None
        if prefix and (self.prefix_slots is None or self.prefix_len is None or self.slots is None):
            raise ValueError("a prefix table needs prefix_slots, prefix_len and a slot table")
        if prefix and (self.variants is not None or self.lora is not None):
            raise ValueError("a prefix table is not served with LoRA variants or a PackedLora")
        if (self.variants is None) != (self.bank is None):
            raise ValueError("a variant table and its bank come together")
        if self.lora is not None and (self.variants is not None or self.slots is not None):
            raise ValueError("a PackedLora is not served with a variant table or a slot table")
        if self.slots is not None and (self.slot0 != 0 or self.n_slots <= 0):
            raise ValueError("a slot table addresses the whole slab: slot0 0, n_slots > 0")

    @staticmethod
    def of(rows: Union[int, "_Rows"]) -> "_Rows":
        return rows if isinstance(rows, _Rows) else _Rows(slot0=int(rows))

    @property
    def kind(self) -> str:
        if self.variants is not None:
            return "_multi_lora"
        if self.lora is not None:
            return "_lora"
        if self.prefix_slots is not None:
            return "_shared"
        return "_slots" if self.slots is not None else ""

    @property
    def plain(self) -> bool:
        """Contiguous slots, no table, no adapter."""
        return self.kind == ""

    forward_entry = property(lambda self: self._ENTRY[self.kind][0])
    forward_ws_entry = property(lambda self: self._ENTRY[self.kind][1])
    step_entry = property(lambda self: self._ENTRY[self.kind][2])
    step_ws_entry = property(lambda self: self._ENTRY[self.kind][3])

    def sub(self, r0: int, r1: int) -> "_Rows":
        """Rows [r0, r1) of the same routing."""
        cut = lambda t: None if t is None else t[r0:r1]
        return replace(self, slot0=self.slot0 if self.slots is not None else self.slot0 + r0, slots=cut(self.slots),
                       prefix_slots=cut(self.prefix_slots), prefix_len=cut(self.prefix_len), variants=cut(self.variants))

    def span(self, b: int) -> int:
        """The slab slots a call over b rows addresses."""
        return self.n_slots if self.slots is not None else self.slot0 + b

    def head(self) -> tuple:
        """The adapter arguments an entry point takes right after the model."""
        if self.variants is not None:
            return self.bank_arg() + (self.variants.data_ptr(),)
        return (self.lora.ptr(),) if self.lora is not None else ()

    def bank_arg(self) -> tuple:
        """The bank argument the workspace functions of a variant table take after the model."""
        return (C.byref(self.bank.struct),) if self.bank is not None else ()

    def tail(self) -> tuple:
        """The table arguments an entry point takes right before the KV struct."""
        if self.slots is None:
            return (None, 0) if self.variants is not None else ()
        out = (self.slots.data_ptr(), self.n_slots)
        return out + (self.prefix_slots.data_ptr(), self.prefix_len.data_ptr()) if self.prefix_slots is not None else out

    def key(self) -> tuple:
        """What a captured graph bakes in of the routing: part of every graph key."""
        return (self.slot0 if self.slots is None else (self.slots.data_ptr(), self.n_slots),
                (self.prefix_slots.data_ptr(), self.prefix_len.data_ptr()) if self.prefix_slots is not None else None,
                (self.variants.data_ptr(), self.bank.generation) if self.variants is not None else None)


def _runs(idx: Sequence[int]) -> List[Tuple[int, int]]:
    """[j0, j1) ranges of ``idx`` (ascending ints) that hold consecutive values."""
    out, j = [], 0
    while j < len(idx):
        k = j
        while k + 1 < len(idx) and idx[k + 1] == idx[k] + 1:
            k += 1
        out.append((j, k + 1))
        j = k + 1
    return out


@dataclass(frozen=True)
class Prepared:
    """What ``_prepare_sequences`` leaves for the decode loop, rows in slot order."""

    order: List[int]           # order[r] = the caller's index of row r
    first: torch.Tensor        # int32 [B]: the first token of each row
    hidden_last: torch.Tensor  # [B, D]: the prompt pass's last hidden row
    next_pos: List[int]
    rows: _Rows                # the routing the decode loop must use
    sampling: Optional[Sampling]  # the call's pick (None: greedy); shared route: ``row_perm`` set; with top-k / min-p: per row
    constraint: Optional[Constraint] = None  # the rows' automata, each past its first token's mask (None: every row free)
    penalty: Optional[Penalty] = None  # the rows' penalties, every history empty (None: every row neutral)
    stop: Optional[Stop] = None  # the rows' stop matchers, nothing fed yet (None: no row has a stop set)
    stop_sets: Optional[List[Optional[stops.StopSet]]] = None  # the rows' stop sets, in slot order like the record

    def in_caller_order(self, per_row: Sequence) -> list:
        out = [None] * len(self.order)
        for r, src in enumerate(self.order):
            out[src] = per_row[r]
        return out

    @property
    def pos(self) -> Union[int, List[int]]:
        """The decode loop's start position: one int when every row has the same."""
        return self.next_pos if len(set(self.next_pos)) > 1 else self.next_pos[0]


class IdTokenizer:
    """Stand-in used when the real vocabulary (``moondream/starmie-v1``) cannot be
    loaded offline: text is a space-separated list of token ids."""

    class _Enc:
        def __init__(self, ids):
            self.ids = ids

    def encode(self, s: str):
        try:
            return self._Enc([int(t) for t in s.split()])
        except ValueError:
            raise ValueError(
                "IdTokenizer only understands space-separated token ids; load the real vocabulary "
                "(tokenizers.Tokenizer 'moondream/starmie-v1') and pass it as tokenizer= for text prompts"
            ) from None

    def decode(self, ids: Iterable[int]) -> str:
        return "".join(f"{int(i)} " for i in ids)


def _load_tokenizer():
    """The reference loads ``moondream/starmie-v1`` from the Hub (moondream.py:89).  Offline that
    fails; the id-echo stand-in is then used, LOUDLY: with it, prompts and outputs are token ids."""
    try:
        from tokenizers import Tokenizer

        return Tokenizer.from_pretrained("moondream/starmie-v1")
    except Exception as e:  # no network / no cache
        import warnings

        warnings.warn(
            f"could not load the 'moondream/starmie-v1' vocabulary ({type(e).__name__}); falling back to IdTokenizer: "
            "text prompts must be space-separated token ids and answers come back as ids.  Pass tokenizer= to avoid this.",
            RuntimeWarning, stacklevel=3,
        )
        return IdTokenizer()


def _is_cjk_char(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF) or (0x3400 <= cp <= 0x4DBF) or (0x2F800 <= cp <= 0x2FA1F)


def _count_crops(v, image: Image.Image) -> int:
    return crop_count(image.size[1], image.size[0], v.overlap_margin, v.max_crops, (v.crop_size, v.crop_size), v.enc_patch_size)[0]


def _crop_into(v, image: Image.Image, out: np.ndarray):
    """Cut the crops of ``image`` (vision config ``v``) into ``out`` [n, crop, crop, 3] uint8 -> (crops, tiling)."""
    arr = np.asarray(image if image.mode == "RGB" else image.convert("RGB"))  # (convert() of an RGB image is a plain copy)
    oc = overlap_crop_image(arr, max_crops=v.max_crops, overlap_margin=v.overlap_margin, base_size=(v.crop_size, v.crop_size),
                            patch_size=v.enc_patch_size, out=out)
    return oc["crops"], tuple(oc["tiling"])


def _crop_pool_workers() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    ranks_here = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1))
    return crop_workers(n, os.cpu_count() or n, ranks_here)


def _capture_graph(body) -> torch.cuda.CUDAGraph:
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def _tree_to_cpu(tree):
    """A nested dict of tensors (a LoRA variant) with every tensor copied to the host."""
    if isinstance(tree, dict):
        return {k: _tree_to_cpu(v) for k, v in tree.items()}
    return tree.detach().to("cpu", copy=True) if isinstance(tree, torch.Tensor) else tree


class MoondreamModel:
    def __init__(
        self,
        config: MoondreamConfig,
        state_dict: Dict[str, torch.Tensor],
        device: Union[str, torch.device] = "cuda",
        dtype: torch.dtype = BF16,
        setup_caches: bool = True,
        tokenizer: Any = None,
        max_batch: int = 1,
        vit_chunk_crops: int = 128,
    ):
        if dtype != BF16:
            raise ValueError("the Moondream hot path is bf16-only (reference: vision.py:36)")
        self.config = config
        self.lib = _lib.load()  # raises when the HIP library has not been built
        self._device = torch.device(device)
        if self._device.type != "cuda":
            raise _lib.MoondreamHipError("MoondreamModel needs a GPU device; there is no CPU path")
        self.tokenizer = tokenizer if tokenizer is not None else _load_tokenizer()
        self._own_vocab_bytes: Optional[List[bytes]] = None  # the tokenizer's vocabulary as bytes (regex_constraint)
        self._vocab_dev_cache: Dict[int, tuple] = {}  # id(vocabulary) -> (vocabulary, tok_off, tok_bytes, n_bytes) on the device
        self._grammar_cache: Dict[tuple, tuple] = {}  # (kind, pattern, id(vocabulary)) -> (vocabulary, TokenAutomaton)
        self.w = PackedModel(config, state_dict, self._device)
        # the checkpoint's own 4-bit weight stream for the decode regime (enable_int4_decode): exact but OPT-IN -- the in-register
        # dequantisation is VALU-bound today (0.82x the bf16 stream's decode phase at B = 64, profiles/r04_int4_weight_stream.txt)
        self.int4_decode = False
        self.vit_chunk_crops = int(vit_chunk_crops)
        self._max_batch = 0
        self._kv_k = self._kv_v = None
        self._kv_k8 = self._kv_v8 = None   # fp8 mode: e4m3 copy of the cache for the decode steps
        self._kv8_scales = None            # (ctypes float[L] for K, for V) when that copy is in use
        # the captured decode graphs and every buffer they bake in but the KV slabs (graph_store.py)
        self._store = GraphStore(partial(torch.cuda.synchronize, self._device), _capture_graph)
        self.use_graphs = False
        self.collect_timing = False
        self.last_phase_ms: Dict[str, float] = {}
        self._region_tables = None
        self._variants: Dict[str, PackedLora] = {}
        self._variant_src: Dict[str, dict] = {}  # registered variants as given (the bank packs its own copy on first use)
        self._bank: Optional[PackedLoraBank] = None  # mixed-variant batches (md_lora_bank)
        # batch-1 greedy decode on the persistent single-sequence kernel (md_decode_step_b1): one launch per token for
        # all decoder blocks; False = the batched kernels at one row (bit-identical to a row of a batch)
        self.single_sequence_kernel = True
        self.strict_batch_invariance = False  # see set_strict_batch_invariance
        # prefills whose caller keeps only the last row of each sequence (or none) skip the last block's work on the other rows
        # (md_text_forward_trim; same bits).  False: the all-rows entry points and a slice -- A/B and tests.
        self.prefill_trim = True
        self._tile_policy = _lib.MD_TILE_BY_SHAPE  # of the call in flight: _select_kernels
        self._b1_sync = None  # barrier state of that kernel: zeroed once, then owned by it
        self._b1_used = False
        # batch_generate over raw images: image prefix + prompt in one decoder pass (False: the reference's two passes).
        # Token generation only: detect / point keep the two passes, so that a raw image and its EncodedImage give the
        # same bits there (the region heads' decisions have no planted margins to absorb a changed accumulation order)
        self.fused_prefill = True
        # encode byte-identical crops of an image once (images that fit one crop: global == local); off = what the reference does
        self.dedup_identical_crops = False
        # resize and tiling on the device (resample.py, md_image_resample_crops): the raw pixels are uploaded and the crops cut
        # there, the same bytes as the host's PIL path.  Opt-in; prefetch_crops and the pipelined engines keep staging on the host
        self._device_preprocess = False
        v = config.vision  # host tiling into pinned buffers: the ring, the pools and the batches staged ahead (crop_staging.py)
        self._staging = CropStager(partial(_count_crops, v), partial(_crop_into, v), (v.crop_size, v.crop_size, 3), _crop_pool_workers)
        if setup_caches:
            self._setup_caches(max_batch)

    # ------------------------------------------------------------------ infra
    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def _graphs(self):
        return self._store.graphs

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    def _h2d(self, t: torch.Tensor) -> torch.Tensor:
        """Small host tensor -> device WITHOUT stalling the host: a copy from pageable memory blocks the calling thread until the
        stream has reached it (on the pipelined engine's streams: until the whole encode in front of it has run); from pinned
        memory it is queued like a kernel."""
        if t.device.type != "cpu":
            return t.to(self._device)
        with torch.inference_mode(False):
            pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        pinned.copy_(t)
        return pinned.to(self._device, non_blocking=True)

    def _setup_caches(self, max_batch: Optional[int] = None):
        """Zeroed KV slabs [L][B][H_kv][ctx][hd] (reference: moondream.py:62-72,152-162)."""
        t = self.config.text
        b = max(1, int(max_batch or self._max_batch or 1))
        old_k, old_v = self._kv_k, self._kv_v
        if old_k is not None:
            # growing: work queued on the pipelined engine's streams may still use the old slabs,
            # arenas and captured graphs
            torch.cuda.synchronize(self._device)
        # ordinary (non-inference) tensors even when a generate call grows the slabs from inside
        # torch.inference_mode(): load_encoded_image updates them in place from user code
        with torch.inference_mode(False):
            self._kv_k = torch.zeros(t.n_layers, b, t.n_kv_heads, t.max_context, t.head_dim, dtype=BF16, device=self._device)
            self._kv_v = torch.zeros_like(self._kv_k)
            old_k8, old_v8 = self._kv_k8, self._kv_v8
            if self._kv8_scales is not None:  # fp8 mode: the e4m3 copy the decode steps read
                self._kv_k8 = torch.zeros(self._kv_k.shape, dtype=torch.uint8, device=self._device)
                self._kv_v8 = torch.zeros_like(self._kv_k8)
            if old_k is not None:  # slots loaded earlier (load_encoded_image) survive the growth
                keep = min(b, old_k.shape[1])
                self._kv_k[:, :keep] = old_k[:, :keep]
                self._kv_v[:, :keep] = old_v[:, :keep]
                if old_k8 is not None and self._kv_k8 is not None:
                    self._kv_k8[:, :keep] = old_k8[:, :keep]
                    self._kv_v8[:, :keep] = old_v8[:, :keep]
        self._max_batch = b
        self._store.invalidate()

    def _ensure_batch(self, b: int):
        if self._kv_k is None or b > self._max_batch:
            self._setup_caches(b)

    def _kv_struct(self, slot0: int = 0) -> _lib.MdKvCache:
        t = self.config.text
        bs = t.n_kv_heads * t.max_context * t.head_dim
        off = slot0 * bs * 2
        kv = _lib.MdKvCache(
            self._kv_k.data_ptr() + off, self._kv_v.data_ptr() + off, self._max_batch * bs, bs, t.max_context
        )
        if self._kv8_scales is not None and self._kv_k8 is not None:
            off8 = slot0 * bs
            kv.k8, kv.v8 = self._kv_k8.data_ptr() + off8, self._kv_v8.data_ptr() + off8
            kv.k_scale = C.cast(self._kv8_scales[0], C.c_void_p)
            kv.v_scale = C.cast(self._kv8_scales[1], C.c_void_p)
        return kv

    def _workspace(self, nbytes: int, which: int = 0) -> torch.Tensor:
        """Caller-owned arenas for the C ABI.  0: encode-side stages, 1: lm_head of the
        prompt prefill, 2: the decode loop (its own arena so that a decode running on
        the decode stream never shares scratch with an encode on the encode stream)."""
        return self._store.grow(("arena", which), nbytes,
                                lambda: torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=self._device))

    @classmethod
    def from_pretrained(cls, weights_file: str, config: Optional[MoondreamConfig] = None, **kwargs):
        """Build the model from a checkpoint file (``.safetensors`` / ``.pt``; both key layouts the
        reference accepts, weights.py:112-171).  ``config`` defaults to the 2B configuration."""
        from .config import get_config
        from .weights import load_state_dict_file

        return cls(config or get_config("2b"), load_state_dict_file(weights_file), **kwargs)

    def register_variant(self, variant_id: str, lora: dict):
        """Make a LoRA variant available to ``settings={"variant": variant_id}`` without the network: ``lora`` is the
        nested dict the reference's ``variant_state_dict`` returns (lora.py:54-79)."""
        self._variants[variant_id] = PackedLora(self.config, lora, self._device)
        # a host copy for the bank (which packs its own device copy on first use); a variant registered again under the same
        # id replaces the bank's copy in place, so that ``variants=`` serves what ``variant=`` serves
        self._variant_src[variant_id] = _tree_to_cpu(lora)
        if self._bank is not None and variant_id in self._bank.index:
            self._bank.add(variant_id, self._variant_src[variant_id], replace=True)

    def _bank_index(self, variant_id: str) -> int:
        """The index of ``variant_id`` in the model's LoRA bank, adding the variant on first use (a registered one, or the
        on-disk cache's as ``settings={"variant": ...}`` finds it: FileNotFoundError when there is none)."""
        if self._bank is None:
            self._bank = PackedLoraBank(self.config, self.w.text, self._device)
        if variant_id not in self._bank.index:
            src = self._variant_src.get(variant_id)
            if src is None:
                src = variant_state_dict(variant_id, device="cpu")
            self._bank.add(variant_id, src)
        return self._bank.index[variant_id]

    def _variant_table(self, rows: Sequence[int]) -> torch.Tensor:
        """The per-sequence variant table of a mixed batch on the device, in one persistent buffer (captured decode graphs
        keep its address)."""
        b = len(rows)
        buf = self._store.grow("variants", b, lambda: torch.empty(max(b, 64), dtype=torch.int32, device=self._device))
        buf[:b].copy_(self._h2d(torch.tensor(list(rows), dtype=torch.int32)))
        return buf[:b]

    def _lora(self, settings: Optional[dict]) -> Optional[PackedLora]:
        """The packed variant named by ``settings["variant"]`` (reference: moondream.py:241-245,455-459), or None."""
        vid = (settings or {}).get("variant")
        if vid is None:
            return None
        if vid not in self._variants:
            self._variants[vid] = PackedLora(self.config, variant_state_dict(vid, device="cpu"), self._device)
        return self._variants[vid]

    def enable_fp8_decode(self, on: bool = True):
        """Opt-in numerical mode (BASELINE configs[4]): every decoder launch of <= 64 rows streams FP8 e4m3fn copies of
        the decoder weights -- half the bytes of the bandwidth-bound decode step -- with bf16 activations and fp32
        accumulation.  That is every decode step, and also any SHORT prefill (a text-only prompt, the prompt pass of the
        two-pass path at batch 1) and the lm_head of a prompt prefill of <= 64 sequences; the 730-row image prefill, the
        vision path and the KV cache stay bf16.  Outputs are judged by tolerance against
        the bf16 path (tests/test_model_gpu.py), not bit parity; off by default."""
        if on:
            if getattr(self.w, "_fp8_is_int4", False):
                self.w.disable_fp8_decode()  # one weight stream at a time: the e4m3 copy replaces the checkpoint's int4 stream
            self.w.enable_fp8_decode()
        else:
            self.w.disable_fp8_decode()
            if self.int4_decode and self.w.has_int4_source():
                self.w.enable_int4_decode()
        self._store.invalidate()  # captured decode steps baked the other launches in

    def enable_int4_decode(self, on: bool = True):
        """A checkpoint that stores the decoder blocks as the reference's QuantizedLinear triples (layers.py:47-109) carries
        its own 4-bit weight stream: decode launches (<= 64 rows) read the nibbles and rebuild the bf16 weights in registers
        with the reference's dequantisation arithmetic -- the SAME weights as the bf16 copy the prefill multiplies with, at a
        quarter of the bytes of the bandwidth-bound step.  Not a numerical mode (the operands are bit-identical), but OPT-IN:
        the rebuild costs ~4 VALU instructions per weight and the first version of the kernel is VALU-bound (decode phase
        0.82x the bf16 stream's at B = 64; profiles/r04_int4_weight_stream.txt).  The single-sequence persistent kernel
        streams bf16 weights only, so a lone sequence then decodes on the batched kernels."""
        self.int4_decode = bool(on)
        self.w.disable_fp8_decode()
        if on:
            if not self.w.has_int4_source():
                raise ValueError("this checkpoint has no QuantizedLinear (int4) decoder blocks")
            self.w.enable_int4_decode()
        self._store.invalidate()

    def enable_fp8(self, calibration_images: Optional[Sequence[Image.Image]] = None, prompt: Optional[Sequence[int]] = None,
                   on: bool = True, decode_weights: bool = True, margin: float = 1.5, kv_cache: bool = True) -> Optional[dict]:
        """Opt-in FP8 mode of the whole hot path (BASELINE configs[4] "fp8 weights, CDNA4 fp8 MFMA"): every MFMA-bound
        linear of the ViT blocks, the projector and the decoder prefill runs on ``md_gemm_f8`` (e4m3 operands,
        v_mfma_f32_32x32x64_f8f6f4 at twice the bf16 matrix rate, fp32 accumulation) with per-channel weight scales and ONE
        static scale per quantised activation tensor; ``decode_weights`` also streams e4m3 weights in the decode steps
        (``enable_fp8_decode``).  Patch embedding, layer-norm statistics, attention, RoPE, the KV cache, the residual
        stream, lm_head at prefill and the region head stay bf16 / fp32.  ``kv_cache`` (needs ``decode_weights``, MHA,
        head_dim 64) additionally keeps an e4m3 COPY of the KV cache, one static scale per layer for K and for V, that the
        decode steps attend over instead of the bf16 slabs -- half the bytes of the step's dominant stream; prefill
        attention, ``EncodedImage`` snapshots and the reference-compatible views keep using the bf16 slabs.

        The activation scales are CALIBRATED: ``calibration_images`` (a handful is enough) are run through the bf16
        path once with range recording on (vision + image / prompt prefill), then the e4m3 weight copies are built.
        The reference has no fp8 path: outputs are judged by tolerance against the bf16 mode (tests/test_model_gpu.py),
        never by bit parity, and the mode is off by default.  Returns the recorded ranges."""
        self._store.invalidate()
        if not on:
            self.w.disable_f8()
            if decode_weights:
                self.enable_fp8_decode(False)
            torch.cuda.synchronize(self._device)
            self._kv8_scales = None
            self._kv_k8 = self._kv_v8 = None
            return None
        if not calibration_images:
            raise ValueError("enable_fp8 needs a few calibration images (PIL) to size the activation scales")
        # a previous call's e4m3 cache copy does not survive this one (kv_cache=False after kv_cache=True must really turn it off)
        self._kv8_scales = None
        self._kv_k8 = self._kv_v8 = None
        tpl = self.config.tokenizer.templates["caption"]
        prompt = list(prompt) if prompt is not None else list(tpl["normal"] if tpl else [self.config.tokenizer.bos_id])
        self.w.begin_f8_calibration()
        try:
            with torch.inference_mode():
                n = len(calibration_images)
                self._prepare_sequences(calibration_images, [prompt] * n, fuse=True)
                torch.cuda.synchronize(self._device)
                t = self.config.text
                p1 = t.prefix_attn + len(prompt)
                # (the e4m3 decode attention keeps a context's scores in LDS: contexts of at most 2048 positions)
                if kv_cache and decode_weights and t.n_heads == t.n_kv_heads and t.head_dim == 64 and t.max_context <= 2048:
                    # K / V ranges of the calibration batch per layer (rows 0 .. p1 - 1 of its slots: the prefill just written)
                    ka = self._kv_k[:, :n, :, :p1].float().abs().amax(dim=(1, 2, 3, 4)).cpu().tolist()
                    va = self._kv_v[:, :n, :, :p1].float().abs().amax(dim=(1, 2, 3, 4)).cpu().tolist()
                    sc = lambda a: (a * margin / 448.0) if a > 0 else 1.0
                    self._kv8_scales = ((C.c_float * t.n_layers)(*[sc(a) for a in ka]), (C.c_float * t.n_layers)(*[sc(a) for a in va]))
                    self._kv_k8 = torch.zeros(self._kv_k.shape, dtype=torch.uint8, device=self._device)
                    self._kv_v8 = torch.zeros_like(self._kv_k8)
                    # slots that already hold sequences (load_encoded_image before this call): their e4m3 rows are built now
                    kv = self._kv_struct(0)
                    _lib.check(self.lib.md_kv_quantize_f8(C.byref(kv), t.n_layers, int(self._kv_k.shape[1]), t.n_kv_heads, None, 0,
                                                          int(t.max_context), self._stream()), "md_kv_quantize_f8")
            info = self.w.finish_f8_calibration(margin)
            info["kv_cache_fp8"] = self._kv8_scales is not None
        except Exception:
            self.w.disable_f8()
            raise
        if decode_weights:
            self.enable_fp8_decode(True)
        return info

    def set_strict_batch_invariance(self, on: bool = True):
        """``on``: every sequence gets the same bits whatever the batch it travels in -- ``batch_generate_ids([a, b, ..])[i]``
        == ``batch_generate_ids([x])`` == ``caption(x)`` bit for bit -- by giving up the two B=1 / batch-level shortcuts whose
        accumulation order differs from the batched kernels': the persistent single-sequence decode kernel (fp32 matrix-vector
        products, per-slice softmax maxima) and the fused [image | prompt] prefill pass (``caption`` / ``query`` make the
        reference's two passes), and by keeping every launch of a short (<= 64-token) prompt pass at <= 64 rows, so that it
        takes the same split-K kernels whether its sequence travels alone or in a batch.  Off (the default) those two are used; outputs then agree with the strict mode within bf16
        accumulation-order noise, i.e. ids can part only at decisions whose top-1/top-2 margin is inside that noise
        (quantified on the 64 bench images by tests/test_model_gpu.py::test_batch_equals_sequential_unfiltered)."""
        self.single_sequence_kernel = not on
        self.fused_prefill = not on
        self.strict_batch_invariance = bool(on)
        self._select_kernels(1)
        self._store.invalidate()

    def _select_kernels(self, n_sequences: int):
        """The library's tile choice by row count would give a lone image (730 / 1458 rows) the small-shape tile configs and a
        batch the four-wave kernel, whose 16x16x32 MFMAs sum K in another association.  Every call is therefore made with the
        tile config PINNED to the layer shape (``tile_policy = MD_TILE_PINNED`` in THIS model's ``md_vit_model`` /
        ``md_text_model`` structs, read by the library per call: ABI 5; no process-wide state, so two models or threads in
        one process do not affect each other's bits) -- so that ``batch_generate_ids(B)[i] == batch_generate_ids([x_i])``
        holds bit for bit in the DEFAULT mode as long as the lone sequence runs on the batched kernels -- except the
        documented latency path: ONE sequence with ``single_sequence_kernel`` on (small-shape tiles at prefill, the persistent
        kernel at decode).  Called by every public entry point that can launch a GEMM of more than 64 rows."""
        pin = (self.strict_batch_invariance or not (n_sequences == 1 and self.single_sequence_kernel))
        self._tile_policy = _lib.MD_TILE_PINNED if pin else _lib.MD_TILE_BY_SHAPE
        self.w.vit.tile_policy = self._tile_policy
        self.w.text.tile_policy = self._tile_policy

    def compile(self):
        """The reference rebinds the seam to torch.compile'd functions here
        (moondream.py:194-204).  The seam is already native; ``compile`` turns on
        hipGraph replay of the device-resident decode step."""
        self.use_graphs = True

    # ------------------------------------------------------------------ seam
    def _vis_enc(self, x: torch.Tensor) -> torch.Tensor:
        """bf16 [N,3,378,378] -> bf16 [N,729,D_v].  reference: moondream.py:168-169."""
        v = self.config.vision
        assert x.dtype == BF16 and x.dim() == 4 and x.shape[1:] == (3, v.crop_size, v.crop_size)
        x = x.contiguous()
        self._select_kernels(1)  # the seam is the reference's one-image-at-a-time path
        return self._vit_run(x, _lib.MD_CROPS_BF16_CHW)

    def _vit_run(self, crops: torch.Tensor, kind: int) -> torch.Tensor:
        v = self.config.vision
        n = crops.shape[0]
        out = torch.empty(n, v.n_patches, v.enc_dim, dtype=BF16, device=self._device)
        chunk = max(1, self.vit_chunk_crops)
        need = self.lib.md_vit_workspace_bytes(C.byref(self.w.vit), min(n, chunk))
        ws = self._workspace(need)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            _lib.check(
                self.lib.md_vit_encode(
                    C.byref(self.w.vit), crops[i : i + m].data_ptr(), kind, m, out[i : i + m].data_ptr(),
                    ws.data_ptr(), ws.numel(), self._stream(),
                ),
                "md_vit_encode",
            )
        return out

    def _vis_proj(self, g: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
        """global [729,D_v] + stitched grid [h,w,D_v] -> [729,D].  reference: moondream.py:171-172."""
        v = self.config.vision
        g, r = g.contiguous(), r.contiguous()
        self._select_kernels(1)
        out = torch.empty(v.n_patches, v.proj_out_dim, dtype=BF16, device=self._device)
        need = self.lib.md_vision_project_workspace_bytes(C.byref(self.w.vit), 1)
        ws = self._workspace(need)
        _lib.check(
            self.lib.md_vision_project_grid(
                C.byref(self.w.vit), g.data_ptr(), r.data_ptr(), r.shape[0], r.shape[1], out.data_ptr(),
                v.proj_out_dim, ws.data_ptr(), ws.numel(), self._stream(),
            ),
            "md_vision_project_grid",
        )
        return out

    def _causal_text_struct(self):
        """The decoder description with an empty bidirectional prefix: the plain causal
        mask the reference builds for a text-only query (moondream.py:571-575)."""
        # rebuilt on every call: a cached byte copy would keep a stale ``fp8`` pointer across
        # enable_fp8_decode / disable_fp8_decode (the library reads the struct on the host, during the call)
        st = type(self.w.text).from_buffer_copy(self.w.text)
        st.prefix_len = 0
        self._text_causal = st
        return st

    def _text_forward(self, x: torch.Tensor, pos0: Union[int, Sequence[int]], rows: Union[int, _Rows] = 0, causal: bool = False,
                      pos_dev: Optional[torch.Tensor] = None, keep: str = "all") -> Optional[torch.Tensor]:
        """x [B,T,D] embeddings -> hidden [B,T,D]; K,V written at pos0[b]..pos0[b]+T-1.
        ``keep``: the hidden rows the caller reads -- "all", "last" (returns [B,1,D], the last row of every sequence: what
        lm_head and the first decode step take from a prefill) or "none" (returns None: the K / V rows are the result).  The
        last two go to md_text_forward_trim, which skips the last block's work on the other rows (``prefill_trim`` off, or
        a LoRA routing: the all-rows entry point and a slice -- the same bits).
        ``pos0`` is host data (one int for the whole batch or one per sequence): the slab has
        max_context slots per head and the kernels do not bounds-check, so the check is here
        (the reference fails at this point too: its index_put / mask indexing raises).
        ``rows``: where the rows live and what adapters they carry (``_Rows``; an int: contiguous from that slot).  A prefix
        table was checked by ``check_shared_table``."""
        rows = _Rows.of(rows)
        b, t, d = x.shape
        if self.strict_batch_invariance and rows.lora is None and pos_dev is None and 1 < t <= 64 and b * t > 64:
            # The library picks the split-K decode-regime kernels by the ROW COUNT of a launch (<= 64 rows), and split-K sums
            # fp32 partials in another association than the sequential-K tile kernels.  A short prompt pass would so take
            # different kernels alone (t rows) and in a batch (b x t rows).  Strict mode keeps every launch of a short pass
            # at <= 64 rows: groups of 64 // t sequences, each through the kernels a lone sequence gets.
            per = max(1, 64 // t)
            outs = []
            for i0 in range(0, b, per):
                p0 = pos0 if isinstance(pos0, int) else list(pos0)[i0 : i0 + per]
                outs.append(self._text_forward(x[i0 : i0 + per], p0, rows.sub(i0, min(b, i0 + per)), causal=causal, keep=keep))
            return None if keep == "none" else torch.cat(outs, dim=0)
        hi = pos0 if isinstance(pos0, int) else max(int(p) for p in pos0)
        lo = pos0 if isinstance(pos0, int) else min(int(p) for p in pos0)
        if lo < 0 or hi + t > self.config.text.max_context:
            raise ValueError(
                f"positions [{lo}, {hi + t}) do not fit the {self.config.text.max_context}-slot context "
                "(image prefix + prompt + generated tokens)"
            )
        if pos_dev is not None:  # the same positions, already on the device (loops that advance them there)
            assert pos_dev.dtype == torch.int32 and pos_dev.numel() == b
            pos0 = pos_dev
        elif isinstance(pos0, int):
            pos0 = torch.full((b,), pos0, dtype=torch.int32, device=self._device)
        else:
            assert len(pos0) == b
            pos0 = self._h2d(torch.tensor([int(p) for p in pos0], dtype=torch.int32))
        for tab in (rows.slots, rows.variants):
            assert tab is None or (tab.dtype == torch.int32 and tab.numel() == b)
        assert not (causal and rows.prefix_slots is not None)
        text = self._causal_text_struct() if causal else self.w.text
        self._ensure_batch(rows.span(b))
        x = x.contiguous()
        hidden = torch.empty_like(x)
        kv = self._kv_struct(rows.slot0)
        ws = self._workspace(getattr(self.lib, rows.forward_ws_entry)(C.byref(text), *rows.bank_arg(), b, t))
        assert keep in ("all", "last", "none")
        if keep != "all" and self.prefill_trim and rows.kind in ("", "_slots", "_shared"):
            last = torch.empty(b, 1, d, dtype=x.dtype, device=x.device) if keep == "last" else None
            tables = [tab.data_ptr() if tab is not None else None for tab in (rows.slots, rows.prefix_slots, rows.prefix_len)]
            _lib.check(
                self.lib.md_text_forward_trim(
                    C.byref(text), x.data_ptr(), hidden.data_ptr(), last.data_ptr() if last is not None else None,
                    _lib.MD_HIDDEN_LAST if keep == "last" else _lib.MD_HIDDEN_NONE, b, t, pos0.data_ptr(), tables[0], rows.n_slots,
                    tables[1], tables[2], C.byref(kv), ws.data_ptr(), ws.numel(), self._stream(),
                ),
                "md_text_forward_trim",
            )
            return last
        # one call site for md_text_forward and its _slots / _shared / _multi_lora (grouped LoRA kernels, csrc/lora_multi.hip) /
        # _lora (unfused kernels + low-rank pairs: text.py:31-32,55-56; layers.py:129-146) forms
        _lib.check(
            getattr(self.lib, rows.forward_entry)(
                C.byref(text), *rows.head(), x.data_ptr(), hidden.data_ptr(), b, t, pos0.data_ptr(), *rows.tail(), C.byref(kv),
                ws.data_ptr(), ws.numel(), self._stream(),
            ),
            rows.forward_entry,
        )
        if keep == "last":
            return hidden[:, -1:, :].contiguous()
        return hidden if keep == "all" else None

    def _decode_ws_bytes(self, rows: _Rows, b: int) -> int:
        """The workspace of a decode step over b rows routed by ``rows``."""
        return getattr(self.lib, rows.step_ws_entry)(C.byref(self.w.text), *rows.bank_arg(), b)

    def _decode_step(self, rows: _Rows, tok_in: torch.Tensor, tok_out: torch.Tensor, pos_buf: torch.Tensor, b: int, suppress_id: int,
                     logits: torch.Tensor, ws: torch.Tensor, kv: _lib.MdKvCache):
        """One device-resident decode step over b rows (embed -> decoder -> lm_head -> suppress + argmax; logits [b, V] left
        in ``logits``): the one call site of md_decode_step and its _slots / _shared / _multi_lora forms."""
        _lib.check(
            getattr(self.lib, rows.step_entry)(
                C.byref(self.w.text), *rows.head(), tok_in.data_ptr(), tok_out.data_ptr(), pos_buf.data_ptr(), b, *rows.tail(),
                C.byref(kv), suppress_id, logits.data_ptr(), self.config.text.vocab_size, ws.data_ptr(), ws.numel(), self._stream(),
            ),
            rows.step_entry,
        )

    def _decode_step_reason(self, rows: _Rows, reason: ReasonChunk, i: int, tok_in: torch.Tensor, pos_buf: torch.Tensor, b: int,
                            logits: torch.Tensor, ws: torch.Tensor, kv: _lib.MdKvCache):
        """Step ``i`` of a reasoning chunk over b rows (md_decode_step_reason): region head on the previous hidden state ->
        each row's input by its phase -> decoder -> lm_head -> the phase's ids masked in ``logits`` [b, V]; the pick is the
        caller's.  Routing: contiguous, a slot table or a shared prefix; no adapters."""
        if rows.kind not in ("", "_slots", "_shared"):
            raise ValueError("the reasoning step is not served with LoRA adapters")
        ptr = lambda t: t.data_ptr() if t is not None else None
        st = _lib.MdReasonState(
            reason.phase.data_ptr(), reason.n_reason.data_ptr(), reason.n_answer.data_ptr(), reason.kind[i].data_ptr(),
            reason.ground[i].data_ptr(), reason.suppress.data_ptr(), reason.coord_bin.data_ptr(), reason.hidden_prev.data_ptr(),
            reason.forced[i].data_ptr() if reason.forced is not None else None, int(reason.max_reason), int(reason.max_answer),
            *self._reason_ids())
        _lib.check(
            self.lib.md_decode_step_reason(
                C.byref(self.w.text), C.byref(reason.region), C.byref(st), None, tok_in.data_ptr(), pos_buf.data_ptr(), b,
                ptr(rows.slots), rows.n_slots, ptr(rows.prefix_slots), ptr(rows.prefix_len), C.byref(kv), logits.data_ptr(),
                self.config.text.vocab_size, ws.data_ptr(), ws.numel(), self._stream(),
            ),
            "md_decode_step_reason",
        )

    def _reason_ids(self) -> Tuple[int, int, int, int, int]:
        """(answer_id, eos_id, size_id, coord_id, suffix_id) of md_reason_state."""
        tk = self.config.tokenizer
        return tk.answer_id, tk.eos_id, tk.size_id, tk.coord_id, int(tk.templates["query"]["suffix"][0])

    def _decode_step_b1(self, tok_in: torch.Tensor, tok_out: torch.Tensor, pos_buf: torch.Tensor, suppress_id: int,
                        logits: torch.Tensor, ws: torch.Tensor, kv: _lib.MdKvCache):
        """``_decode_step`` of ONE sequence, greedy, plain contiguous routing, as one persistent launch (csrc/decode_b1.hip)."""
        st = self.lib.md_decode_step_b1(
            C.byref(self.w.text), tok_in.data_ptr(), tok_out.data_ptr(), pos_buf.data_ptr(), C.byref(kv), suppress_id,
            logits.data_ptr(), self.config.text.vocab_size, ws.data_ptr(), ws.numel(), self._b1_sync.data_ptr(), self._stream())
        _lib.check(st, "md_decode_step_b1")

    def _step_from_pieces(self, x: torch.Tensor, pos: Union[int, Sequence[int]], rows: Union[int, _Rows] = 0,
                          pos_dev: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One decode step from its pieces, for what the fused step does not serve (a LoRA adapter, an embedding that is not
        a token's, a host decision per token): ``x`` token ids (integer [B, 1]) or embeddings [B, 1, D] -> decoder at ``pos``
        -> lm_head.  Returns (hidden [B, 1, D], logits [B, V]); the pick is the caller's."""
        hidden = self._text_forward(x if x.is_floating_point() else self._embed(x), pos, rows, pos_dev=pos_dev)
        return hidden, self._lm_head(hidden)

    def _lm_head(self, hidden: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hidden [B,T,D] -> logits of the last token [B,V] (into ``out`` when given).  reference: text.py:163-167."""
        b, t, d = hidden.shape
        logits = out if out is not None else torch.empty(b, self.config.text.vocab_size, dtype=BF16, device=self._device)
        assert logits.shape == (b, self.config.text.vocab_size) and logits.dtype == BF16 and logits.stride(1) == 1
        need = self.lib.md_lm_head_workspace_bytes(C.byref(self.w.text), b)
        ws = self._workspace(need, 1)
        _lib.check(
            self.lib.md_lm_head(
                C.byref(self.w.text), hidden.contiguous().data_ptr(), b, t, logits.data_ptr(), logits.stride(0),
                ws.data_ptr(), ws.numel(), self._stream(),
            ),
            "md_lm_head",
        )
        return logits

    def _seam_rule(self, attn_mask: Optional[torch.Tensor], pos_ids: torch.Tensor, t: int):
        """(first position, causal?) for the mask slice and positions the reference passes through the seam
        (moondream.py:304-309: a slice of the prefix-LM buffer; 571-575: of a plain tril for the text-only query;
        472-474,515: the decode row).  Any other mask, and non-consecutive positions, raise ValueError."""
        if int(pos_ids.numel()) != t:
            raise ValueError(f"pos_ids has {int(pos_ids.numel())} entries for {t} embedding row(s)")
        tc = self.config.text
        kind = classify_attn_mask(attn_mask, pos_ids, tc.prefix_attn, tc.max_context)
        pos0 = int(pos_ids.reshape(-1)[0])
        if attn_mask is None and pos0 < tc.prefix_attn:
            kind = MASK_PREFIX_LM  # None = the prefix-LM buffer's slice (moondream.py:303-304): same check as an explicit one
        if kind == MASK_PREFIX_LM and pos0 + t < tc.prefix_attn:
            # such a slice lets its rows see keys [pos0 + t, prefix) that this pass does not write; the library reads keys
            # [0, pos0 + t) only.  The reference always prefills the whole prefix in one pass (moondream.py:254-258).
            raise ValueError(f"a prefix-LM pass must reach the end of the {tc.prefix_attn}-position bidirectional prefix "
                             f"(got positions [{pos0}, {pos0 + t}))")
        return pos0, kind == MASK_CAUSAL

    def _prefill(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor], pos_ids: torch.Tensor, lora=None):
        """reference: moondream.py:174-181.  x [1,T,D]; attn_mask bool [1,1,T,ctx] (or None = the prefix-LM buffer's
        slice); pos_ids int64 [T] consecutive.  The mask is CLASSIFIED, not applied: the prefix-LM slice and the plain
        causal slice (text-only query) select the library's two rules; anything else is a ValueError."""
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"x must be [1, T, D] (got {tuple(x.shape)})")
        pos0, causal = self._seam_rule(attn_mask, pos_ids, int(x.shape[1]))
        self._select_kernels(1)
        return self._text_forward(x.to(self._device), pos0, _Rows(lora=lora), causal=causal)

    def _decode_one_tok(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor], pos_ids: torch.Tensor, lora=None):
        """reference: moondream.py:183-192.  x [1,1,D], attn_mask bool [1,1,ctx] with ones on [0, pos] ->
        (logits [1,V], hidden [1,1,D])."""
        hidden = self._prefill(x, attn_mask, pos_ids, lora)
        return self._lm_head(hidden), hidden

    # ------------------------------------------------------------ vision path
    def _embed(self, ids: torch.Tensor) -> torch.Tensor:
        """token ids [..] -> embeddings [.., D]  (reference: text.py:12-13)."""
        if ids.device.type == "cpu" and ids.numel():  # user-supplied prompt ids: the gather kernel does not range-check
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.config.text.vocab_size:
                raise ValueError(f"token id out of range [0, {self.config.text.vocab_size}): {lo if lo < 0 else hi}")
        flat = self._h2d(ids.reshape(-1).to(torch.int32).contiguous())
        d = self.config.text.dim
        out = torch.empty(flat.numel(), d, dtype=BF16, device=self._device)
        _lib.check(
            self.lib.md_embed_tokens(flat.data_ptr(), self.w.wte.data_ptr(), d, out.data_ptr(), d, flat.numel(), d, self._stream()),
            "md_embed_tokens",
        )
        return out.reshape(*ids.shape, d)

    def _crop(self, image: Image.Image):
        v = self.config.vision
        arr = np.array(image.convert("RGB"))
        oc = overlap_crop_image(arr, max_crops=v.max_crops, overlap_margin=v.overlap_margin)
        return oc["crops"], tuple(oc["tiling"])

    @property
    def device_preprocess(self) -> bool:
        """Resize and tile images on the device (PIL-exact; resample.py).  Off by default."""
        return self._device_preprocess

    @device_preprocess.setter
    def device_preprocess(self, on: bool) -> None:
        if on and resize_backend() != "pil":
            raise ValueError("device_preprocess implements the PIL resize only and this process resizes with pyvips: "
                             "start it with MOONDREAM_RESIZE=pil")
        self._device_preprocess = bool(on)

    def _device_plan(self, images: Sequence[Image.Image]):
        """The images' resample.plan records when this call is preprocessed on the device, else None: the switch is off,
        host crops of exactly these images were prefetched, or an image is outside the device path's limits."""
        if not self._device_preprocess or tuple(id(im) for im in images) in self._staging.prefetched:
            return None
        return resample.plan([(im.size[1], im.size[0]) for im in images], self.config.vision)

    def _encode_crops_on_device(self, images: Sequence[Image.Image], records, mark=None) -> torch.Tensor:
        """The device form of the loop below: per ViT chunk ONE upload of [descriptors | tables | raw RGB pixels], the two
        resample launches that cut the crops, the ViT."""
        v, ring = self.config.vision, self._staging.ring
        dedup = self.dedup_identical_crops
        feat_parts = []
        for ci, (i0, i1, _) in enumerate(plan_chunks([r.n_crops for r in records], self.vit_chunk_crops)):
            lay = resample.layout(records[i0:i1], v, dedup=dedup)
            with ring.take(lay.nbytes) as lease:  # taken over by its upload, or given back here
                lay.write(lease.array((lay.nbytes,)),
                          [np.asarray(im if im.mode == "RGB" else im.convert("RGB")) for im in images[i0:i1]])
                if mark is not None and ci == 0:
                    mark("host_tiling")  # (the same key as the host path: what the host does before the GPU has work)
                packed = lease.upload(self._device)
            crops = torch.empty(lay.out_crops, v.crop_size, v.crop_size, 3, dtype=torch.uint8, device=self._device)
            ws = self._workspace(self.lib.md_image_resample_workspace_bytes(lay.desc.ctypes.data, i1 - i0))
            crop, window, margin_px = resample.geometry(v)
            _lib.check(
                self.lib.md_image_resample_crops(
                    packed.data_ptr(), packed.numel(), lay.desc.ctypes.data, i1 - i0, crop, window, margin_px,
                    crops.data_ptr(), lay.out_crops, ws.data_ptr(), ws.numel(), self._stream(),
                ),
                "md_image_resample_crops",
            )
            f = self._vit_run(crops, _lib.MD_CROPS_U8_HWC)
            if lay.expand is not None:
                f = f[torch.tensor(lay.expand, dtype=torch.int64, device=self._device)]
            feat_parts.append(f)
        feats = feat_parts[0] if len(feat_parts) == 1 else torch.cat(feat_parts, dim=0)
        # (_project_by_tiling reads an image's crop count and tiling: no host pixels exist on this path)
        return self._project_by_tiling(feats, [(np.broadcast_to(np.uint8(0), (r.n_crops,)), r.tiling) for r in records])

    def _run_vision_encoder_batch(self, images: Sequence[Image.Image], mark=None, staged=None) -> torch.Tensor:
        """images -> [B,729,D] projected embeddings (reference: moondream.py:206-228, per image).

        Host tiling (PIL, reference image_crops.py:58-167) runs on a thread pool and is pipelined against the GPU
        (crop_staging.py): the ViT of image chunk k is enqueued (async) while the crops of chunk k+1 are still being cut.
        ``staged``: these images' StagedBatch when the caller started it ahead; otherwise a prefetched one, or one made now.
        With ``device_preprocess`` on and nothing staged ahead, resize and tiling run on the device instead."""
        if staged is None:
            records = self._device_plan(images)
            if records is not None:
                return self._encode_crops_on_device(list(images), records, mark)
            staged = self._staging.take(images, self.vit_chunk_crops)
        cropped: List[Tuple[np.ndarray, Tuple[int, int]]] = []
        feat_parts = []
        with staged:  # whatever raises in here, the chunks not consumed yet give their buffers back
            for ci in range(len(staged.chunks)):
                part, lease = staged.next_chunk()
                with lease:  # the chunk's buffer is this block's: taken over by its upload, or given back here
                    if mark is not None and ci == 0:
                        mark("host_tiling")  # phase timing: the GPU has nothing of this batch to run before the first crops exist
                    cropped.extend(part)
                    if self.dedup_identical_crops:  # opt-in: the reference encodes both crops of an image that fits one
                        dev_crops, expand = upload_unique(self._staging.ring, part, self._staging.crop_shape, self._device)
                    else:
                        dev_crops, expand = lease.upload(self._device), None
                f = self._vit_run(dev_crops, _lib.MD_CROPS_U8_HWC)
                if expand is not None and len(expand) != dev_crops.shape[0]:
                    f = f[torch.tensor(expand, dtype=torch.int64, device=self._device)]
                feat_parts.append(f)
        feats = feat_parts[0] if len(feat_parts) == 1 else torch.cat(feat_parts, dim=0)  # [sum crops, 729, Dv]
        return self._project_by_tiling(feats, cropped)

    def _project_by_tiling(self, feats: torch.Tensor, cropped) -> torch.Tensor:
        """Encoder features of all crops [sum crops, 729, Dv] + each image's (crops, tiling) -> [B,729,D]: images with the
        same tiling are projected together."""
        v = self.config.vision
        out = torch.empty(len(cropped), v.n_patches, v.proj_out_dim, dtype=BF16, device=self._device)
        offsets, off = [], 0
        for c, _ in cropped:
            offsets.append(off)
            off += c.shape[0]
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, (_, tiling) in enumerate(cropped):
            groups.setdefault(tiling, []).append(i)
        for tiling, idxs in groups.items():
            nc = 1 + tiling[0] * tiling[1]
            contiguous = idxs == list(range(idxs[0], idxs[0] + len(idxs))) and len(groups) == 1
            if contiguous:
                f = feats
            else:
                f = torch.cat([feats[offsets[i] : offsets[i] + nc] for i in idxs], dim=0)
            o = out if contiguous else torch.empty(len(idxs), v.n_patches, v.proj_out_dim, dtype=BF16, device=self._device)
            need = self.lib.md_vision_project_workspace_bytes(C.byref(self.w.vit), len(idxs))
            ws = self._workspace(need)
            _lib.check(
                self.lib.md_vision_project(
                    C.byref(self.w.vit), f.data_ptr(), len(idxs), tiling[0], tiling[1], v.overlap_margin,
                    o.data_ptr(), v.proj_out_dim, ws.data_ptr(), ws.numel(), self._stream(),
                ),
                "md_vision_project",
            )
            if not contiguous:
                out[torch.tensor(idxs, device=self._device)] = o
        return out

    prefetch_workers = 4

    def prefetch_crops(self, images: Sequence[Image.Image]) -> None:
        """Start the host tiling of a batch NOW (thread pool, pinned staging buffers) so that a later call that encodes
        exactly these image objects -- ``batch_detect``, ``batch_generate_ids``, ... -- finds its crops cut: a serving
        loop calls this for batch k+1 before it runs batch k, which hides the PIL resize of large images behind the
        GPU (the pipelined caption engine does the same by construction).  Results are identical."""
        self._staging.prefetch(images, self.vit_chunk_crops, self.prefetch_workers)

    def wait_prefetched_crops(self) -> None:
        """Block until every prefetched batch's crops are cut (tests, benchmarks: a steady-state serving loop never waits)."""
        self._staging.wait_prefetched()

    def discard_prefetched_crops(self, key=None) -> None:
        """Drop prefetched batches that were never encoded (waits for their workers, returns the pinned buffers)."""
        self._staging.discard(key)

    @property
    def _prefetched_crops(self):
        return self._staging.prefetched

    def _run_vision_encoder(self, image: Image.Image) -> torch.Tensor:
        self._select_kernels(1)
        return self._run_vision_encoder_batch([image])[0]

    def _prefill_images(self, img_emb: torch.Tensor, rows: Union[int, _Rows] = 0) -> int:
        """[B,729,D] -> image prefix in the KV slabs of the slots of ``rows``; returns pos (730)."""
        b = img_emb.shape[0]
        bos = self._embed(torch.full((b, 1), self.config.tokenizer.bos_id, dtype=torch.int32))
        x = torch.cat([bos, img_emb], dim=1)
        self._text_forward(x, 0, rows, keep="none")
        return x.shape[1]

    def encode_image(self, image: Union[Image.Image, EncodedImage], settings: Optional[dict] = None) -> EncodedImage:
        """reference: moondream.py:230-268."""
        if isinstance(image, EncodedImage):
            return image
        if not isinstance(image, Image.Image):
            raise ValueError("image must be a PIL Image or EncodedImage")
        lora = self._lora(settings)  # the image prefix depends on the variant (moondream.py:241-257)
        with torch.inference_mode():
            self._ensure_batch(1)
            pos = self._prefill_images(self._run_vision_encoder(image)[None], _Rows(lora=lora))
            caches = [
                (self._kv_k[l, 0:1, :, :pos, :].clone(), self._kv_v[l, 0:1, :, :pos, :].clone())
                for l in range(self.config.text.n_layers)
            ]
        return EncodedImage(pos=pos, caches=caches)

    def load_encoded_image(self, encoded_image: EncodedImage, slot: int = 0):
        """reference: moondream.py:620-623."""
        self._ensure_batch(slot + 1)
        with torch.inference_mode():
            for l, (k, v) in enumerate(encoded_image.caches):
                self._kv_k[l, slot : slot + 1, :, : k.size(2), :] = k
                self._kv_v[l, slot : slot + 1, :, : v.size(2), :] = v
            if self._kv8_scales is not None:  # fp8 mode: rebuild the e4m3 copy of the rows just loaded
                kv = self._kv_struct(slot)
                t = self.config.text
                _lib.check(self.lib.md_kv_quantize_f8(C.byref(kv), t.n_layers, 1, t.n_kv_heads, None, 0, int(encoded_image.pos), self._stream()),
                           "md_kv_quantize_f8")

    # --------------------------------------------------------------- sampling
    def _pick(self, logits: torch.Tensor, temperature: float, top_p: float, suppress_id: int = -1,
              generator: Optional[torch.Generator] = None, probs_out: Optional[torch.Tensor] = None,
              row_perm: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B,V] -> int32 [B]   (reference: moondream.py:313-318,521-528).  Greedy: argmax, ties to the
        lowest id.  Otherwise temperature + top-p on the device (md_sample_top_p): the reference's
        softmax / _apply_top_p / multinomial semantics with one uniform per sequence from torch's
        generator (same distribution as torch.multinomial, different random stream).  ``uniforms`` (device fp32 [B]): the
        caller's draws instead; with ``out`` (device int32 [B]) as well nothing is allocated (captured decode steps)."""
        b, v = logits.shape
        nxt = out if out is not None else torch.empty(b, dtype=torch.int32, device=self._device)
        if temperature == 0:
            _lib.check(
                self.lib.md_argmax_bf16(logits.data_ptr(), logits.stride(0), b, v, suppress_id, nxt.data_ptr(), self._stream()),
                "md_argmax_bf16",
            )
            return nxt
        u = uniforms
        if u is None:
            u = torch.rand(b, device=self._device, dtype=torch.float32, generator=generator)
            if row_perm is not None:  # row i draws the uniform of row row_perm[i] (the shared-prefix rows in the copy path's order)
                u = u[row_perm]
        _lib.check(
            self.lib.md_sample_top_p(
                logits.data_ptr(), logits.stride(0), b, v, suppress_id, float(temperature), float(top_p), u.data_ptr(),
                nxt.data_ptr(), probs_out.data_ptr() if probs_out is not None else None,
                probs_out.stride(0) if probs_out is not None else 0, self._stream(),
            ),
            "md_sample_top_p",
        )
        return nxt

    def _pick_rows(self, logits: torch.Tensor, temperature_dev: torch.Tensor, top_p_dev: torch.Tensor, suppress_id: int,
                   uniforms: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``_pick`` with every row's own settings (md_sample_rows): ``temperature_dev``, ``top_p_dev`` and ``uniforms`` are
        device fp32 [B].  A row of temperature > 0 is drawn as ``_pick`` draws it with those scalars and that uniform, a row
        of temperature 0 takes its argmax, a row of temperature < 0 keeps what ``out`` holds.  With ``out`` (device int32 [B])
        nothing is allocated (captured decode steps)."""
        b, v = logits.shape
        for t in (temperature_dev, top_p_dev, uniforms):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == b and t.device == logits.device
        nxt = out if out is not None else torch.empty(b, dtype=torch.int32, device=self._device)
        _lib.check(
            self.lib.md_sample_rows(logits.data_ptr(), logits.stride(0), b, v, suppress_id, temperature_dev.data_ptr(),
                                    top_p_dev.data_ptr(), uniforms.data_ptr(), nxt.data_ptr(), None, 0, self._stream()),
            "md_sample_rows",
        )
        return nxt

    def _pick_rows_filtered(self, logits: torch.Tensor, temperature_dev: torch.Tensor, top_p_dev: torch.Tensor,
                            top_k_dev: torch.Tensor, min_p_dev: torch.Tensor, suppress_id: int, uniforms: torch.Tensor,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``_pick_rows`` with every row's two further truncation rules (md_sample_rows_filtered): ``top_k_dev`` device int32
        [B], ``min_p_dev`` device fp32 [B].  A sampled row keeps the shortest of its three prefixes of the descending
        order -- top-p's, its first ``top_k`` tokens, the tokens of probability >= min_p * the best one's -- all judged on
        the same unrenormalised distribution; a row of (0, 0) is ``_pick_rows``' row bit for bit; greedy and idle rows read
        neither.  With ``out`` nothing is allocated (captured decode steps)."""
        b, v = logits.shape
        for t in (temperature_dev, top_p_dev, min_p_dev, uniforms):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == b and t.device == logits.device
        assert top_k_dev.dtype == torch.int32 and top_k_dev.is_contiguous() and top_k_dev.numel() == b and top_k_dev.device == logits.device
        nxt = out if out is not None else torch.empty(b, dtype=torch.int32, device=self._device)
        _lib.check(
            self.lib.md_sample_rows_filtered(logits.data_ptr(), logits.stride(0), b, v, suppress_id, temperature_dev.data_ptr(),
                                             top_p_dev.data_ptr(), top_k_dev.data_ptr(), min_p_dev.data_ptr(), uniforms.data_ptr(),
                                             nxt.data_ptr(), None, 0, self._stream()),
            "md_sample_rows_filtered",
        )
        return nxt

    def _filter_record(self, sampling: Optional[Sampling], rows: Optional[Sequence[Tuple[int, float]]]) -> Optional[Sampling]:
        """A call's sampling settings with ``check_filters``' pairs, one per row in the decode loop's row order -> the
        per-row ``Sampling`` record that carries them (every row the call's temperature and top-p, its own top-k and
        min-p; the call's generator and draw order kept).  ``sampling`` itself for no pairs, or for a greedy call: the
        filters cut a sampled row only.  The buffers are the store's, one set per row count: captured chunks keep their
        addresses."""
        if rows is None or sampling is None:
            return sampling
        b = len(rows)
        f, k = self._store.fixed("filters", b, lambda: (torch.empty(3, b, dtype=torch.float32, device=self._device),
                                                        torch.empty(b, dtype=torch.int32, device=self._device)))
        f.copy_(self._h2d(torch.tensor([[float(sampling.temperature)] * b, [float(sampling.top_p)] * b, [r[1] for r in rows]],
                                       dtype=torch.float32)))
        k.copy_(self._h2d(torch.tensor([r[0] for r in rows], dtype=torch.int32)))  # (``check_filters``: below 2^31)
        return replace(sampling, temperature=f[0], top_p=f[1], top_k=k, min_p=f[2])

    def _penalize(self, logits: torch.Tensor, tok_in: torch.Tensor, rows: "_Rows", pen: Penalty):
        """Every row's consumed token ``tok_in[r]`` (device int32 [B]) joins its history in ``pen`` and the logits [B, V] of
        the tokens in that history take the row's penalties in place: md_penalize_rows.  A row's history is its own, or
        (``pen.by_slot``) that of its KV slot in ``rows``; an idle row is left alone.  Nothing is allocated and nothing
        synchronises: capturable."""
        b, v = logits.shape
        assert tok_in.dtype == torch.int32 and tok_in.is_contiguous() and tok_in.numel() == b and tok_in.device == logits.device
        for t in (pen.repetition, pen.presence, pen.frequency):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == b and t.device == logits.device
        assert pen.hist.dtype == torch.int32 and pen.hist_len.dtype == torch.int32 and pen.hist.is_contiguous()
        assert pen.hist.shape == (pen.hist_len.numel(), pen.hist_cap)
        slots = rows.slots if pen.by_slot else None
        assert slots is not None or pen.hist_len.numel() >= b
        _lib.check(
            self.lib.md_penalize_rows(logits.data_ptr(), logits.stride(0), b, v, tok_in.data_ptr(),
                                      slots.data_ptr() if slots is not None else None, 0, pen.hist.data_ptr(), pen.hist_cap,
                                      pen.hist_len.data_ptr(), pen.repetition.data_ptr(), pen.presence.data_ptr(),
                                      pen.frequency.data_ptr(), self._stream()),
            "md_penalize_rows",
        )

    def _penalty_record(self, rows: Optional[Sequence[Tuple[float, float, float]]]) -> Optional[Penalty]:
        """``check_penalties``' triples, one per row in the decode loop's row order -> the ``Penalty`` record of a lockstep
        decode with every history empty (None for None).  The buffers are the store's, one set per row count: captured
        chunks keep their addresses."""
        if rows is None:
            return None
        b, cap = len(rows), min(self.config.text.max_context, _lib.MD_PENALTY_HIST_MAX)  # (more than a row can generate)
        st, hist, hist_len = self._store.fixed("penalty", b, lambda: (
            torch.empty(3, b, dtype=torch.float32, device=self._device),
            torch.zeros(b, cap, dtype=torch.int32, device=self._device), torch.zeros(b, dtype=torch.int32, device=self._device)))
        st.copy_(self._h2d(torch.tensor(rows, dtype=torch.float32).t().contiguous()))
        hist_len.zero_()
        return Penalty(st[0], st[1], st[2], hist, hist_len, cap)

    def _constrain(self, logits: torch.Tensor, tok_in: Optional[torch.Tensor], rows: "_Rows", con: Constraint, row0: int = 0):
        """Every row's automaton in ``con`` is advanced by its consumed token ``tok_in[r]`` (device int32 [B]; None: nothing
        consumed yet, the first token's mask) and the logits [B, V] of the tokens its new state forbids become -inf in
        place: md_constrain_rows.  Row r's state is entry ``row0 + r``, or (``con.by_slot``) that of its KV slot in
        ``rows``; an idle, free or dead row is left alone.  Nothing is allocated and nothing synchronises: capturable."""
        b, v = logits.shape
        assert tok_in is None or (tok_in.dtype == torch.int32 and tok_in.is_contiguous() and tok_in.numel() == b
                                  and tok_in.device == logits.device)
        for t in (con.row_ptr, con.default_next, con.edge_tok, con.edge_next, con.state):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == logits.device
        assert con.row_ptr.numel() == con.state_cap + 1 and con.default_next.numel() == con.state_cap
        slots = rows.slots if con.by_slot else None
        assert slots is not None or con.state.numel() >= row0 + b
        _lib.check(
            self.lib.md_constrain_rows(logits.data_ptr(), logits.stride(0), b, v, tok_in.data_ptr() if tok_in is not None else None,
                                       slots.data_ptr() if slots is not None else None, row0, con.state.data_ptr(),
                                       con.row_ptr.data_ptr(), con.default_next.data_ptr(), con.edge_tok.data_ptr(),
                                       con.edge_next.data_ptr(), con.state_cap, self._stream()),
            "md_constrain_rows",
        )

    def _constraint_record(self, rows: Optional[Sequence[Optional[TokenAutomaton]]]) -> Optional[Constraint]:
        """``check_constraints``' entries, one per row in the decode loop's row order -> the ``Constraint`` record of a
        lockstep decode with every row in its start state and a free row FREE (None for None).  The call's DISTINCT automata
        (by identity) are packed into one table.  The buffers are the store's, one set per (row count, state capacity,
        edge capacity) with the capacities rounded up to powers of two: calls with tables of similar size share their
        addresses and with them their captured chunks.  One pinned copy uploads states and table together."""
        if rows is None:
            return None
        distinct: Dict[int, TokenAutomaton] = {}
        for a in rows:
            if a is not None:
                distinct.setdefault(id(a), a)
        table = pack(list(distinct.values()))
        start = dict(zip(distinct, table.starts))
        b, s_cap, e_cap = len(rows), pow2_at_least(table.n_states), pow2_at_least(table.n_edges)
        buf = self._store.fixed("constraint", (b, s_cap, e_cap), lambda: torch.empty(
            b + 2 * s_cap + 1 + 2 * e_cap, dtype=torch.int32, device=self._device))
        host = np.zeros(buf.numel(), dtype=np.int32)
        state, row_ptr, default_next, edge_tok, edge_next = np.split(host, np.cumsum([b, s_cap + 1, s_cap, e_cap]))
        state[:] = [FREE if a is None else start[id(a)] for a in rows]
        row_ptr[:] = table.n_edges  # the states past the table's own list nothing
        row_ptr[: table.n_states + 1] = table.row_ptr
        default_next[:] = FREE
        default_next[: table.n_states] = table.default_next
        edge_tok[: table.n_edges], edge_next[: table.n_edges] = table.edge_tok, table.edge_next
        buf.copy_(self._h2d(torch.from_numpy(host)))
        d_state, d_row_ptr, d_default, d_tok, d_next = torch.split(buf, [b, s_cap + 1, s_cap, e_cap, e_cap])
        return Constraint(d_row_ptr, d_default, d_tok, d_next, d_state, s_cap)

    def choice_constraint(self, strings: Sequence[str]) -> TokenAutomaton:
        """The automaton that makes a request answer with exactly one of ``strings`` and then stop: each string's token
        ids by the model's tokenizer, as a trie, each followed by ``eos_id`` (``TokenAutomaton.choices``).  For
        ``constraints=`` / ``settings={"constraints": ...}`` of the generation calls."""
        return TokenAutomaton.choices([list(self.tokenizer.encode(s).ids) for s in strings], self.config.tokenizer.eos_id)

    def regex_constraint(self, pattern: str, vocab_bytes: Optional[Sequence[bytes]] = None) -> TokenAutomaton:
        """The automaton under which a request's output spells a full match of ``pattern`` and may stop (eos) only where
        the pattern is complete (moondream_amd/grammar.py: ``compile_regex``; the DFA on the host, the lift over the
        vocabulary on the device).  ``vocab_bytes[v]``: the bytes token v spells, one entry per id of the model's
        vocabulary; None: derived from the model's ``tokenizers.Tokenizer`` (``get_vocab()`` and the GPT-2 byte table).
        The tokenizer's special ids and ``answer_id`` are never allowed.  Cached per (pattern, vocabulary object).
        ValueError for what ``regex_to_dfa`` refuses, a vocabulary of the wrong length, the ``IdTokenizer`` stand-in without
        ``vocab_bytes``, and a pattern this vocabulary cannot spell."""
        return self._grammar_constraint("regex", pattern, vocab_bytes)

    def json_constraint(self, schema: dict, vocab_bytes: Optional[Sequence[bytes]] = None) -> TokenAutomaton:
        """``regex_constraint`` for the compact JSON documents of ``schema`` (``json_schema_to_regex``: its supported subset)."""
        return self._grammar_constraint("json_schema", schema, vocab_bytes)

    def _vocab_bytes(self, kind: str, vocab_bytes: Optional[Sequence[bytes]]) -> Sequence[bytes]:
        """The bytes of every id for ``kind`` ("regex", "json_schema", "stop"): ``vocab_bytes``, or, None, those of the
        model's ``tokenizers.Tokenizer`` (derived once).  ValueError for the ``IdTokenizer`` stand-in without
        ``vocab_bytes`` and for a vocabulary of the wrong length."""
        v = self.config.text.vocab_size
        if vocab_bytes is None:
            if isinstance(self.tokenizer, IdTokenizer):
                raise ValueError(f"{kind}: the IdTokenizer stand-in spells no bytes; pass vocab_bytes (one bytes object per token id)")
            if self._own_vocab_bytes is None:
                self._own_vocab_bytes = grammar.vocab_bytes_of(self.tokenizer, v)
            vocab_bytes = self._own_vocab_bytes
        if len(vocab_bytes) != v:
            raise ValueError(f"vocab_bytes: {len(vocab_bytes)} entries for a vocabulary of {v}")
        return vocab_bytes

    def _vocab_on_device(self, vocab_bytes: Sequence[bytes]):
        """``(tok_off int32 [V + 1], tok_bytes uint8, n_bytes)`` of ``grammar.vocab_arrays`` on the device, uploaded once
        per vocabulary OBJECT (the object is kept, so that its id stays its own); the last four are kept."""
        hit = self._vocab_dev_cache.get(id(vocab_bytes))
        if hit is None or hit[0] is not vocab_bytes:
            off, data = grammar.vocab_arrays(vocab_bytes)
            hit = (vocab_bytes, self._h2d(torch.from_numpy(off)), self._h2d(torch.from_numpy(data.copy())), int(off[-1]))
            while len(self._vocab_dev_cache) >= 4:  # bounded: a caller that makes a new list per call pins at most four
                self._vocab_dev_cache.pop(next(iter(self._vocab_dev_cache)))
            self._vocab_dev_cache[id(vocab_bytes)] = hit
        return hit[1:]

    def _stop_rows(self, tokens: torch.Tensor, rows: "_Rows", stop: Stop):
        """Every row's just-picked token ``tokens[r]`` (device int32 [B]) goes through its stop matcher in ``stop``:
        md_stop_rows.  A row's words are its own, or (``stop.by_slot``) those of its KV slot in ``rows``; an idle row and a
        row without a stop set are left alone.  Nothing is allocated and nothing synchronises: capturable."""
        b = tokens.numel()
        assert tokens.dtype == torch.int32 and tokens.is_contiguous() and tokens.device == stop.words.device
        w = stop.words
        assert w.dtype == torch.int32 and w.is_contiguous() and w.shape[0] == 6
        for t in (stop.match_id, stop.id_ptr, stop.ids, stop.id_base):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == w.device
        assert stop.trans.numel() == stop.state_cap * 256 and stop.match_len.numel() == stop.state_cap and stop.match_id.numel() == stop.state_cap
        assert stop.id_ptr.numel() == w.shape[1] + 1 and stop.id_base.numel() == w.shape[1]
        slots = rows.slots if stop.by_slot else None
        assert slots is not None or w.shape[1] >= b
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(
            self.lib.md_stop_rows(tokens.data_ptr(), b, ptr(slots), 0, stop.trans.data_ptr(), stop.match_len.data_ptr(),
                                  stop.match_id.data_ptr(), stop.state_cap, stop.id_ptr.data_ptr(), stop.ids.data_ptr(),
                                  stop.id_base.data_ptr(), ptr(stop.tok_off), ptr(stop.tok_bytes), stop.vocab, stop.n_bytes,
                                  *(w[i].data_ptr() for i in range(6)), self._stream()),
            "md_stop_rows",
        )

    def _stop_record(self, rows: Optional[Sequence[Optional[stops.StopSet]]], vocab_bytes=None) -> Optional[Stop]:
        """``check_stops``' entries, one per row in the decode loop's row order -> the ``Stop`` record of a lockstep decode
        with every row at its stop set's root, nothing seen and nothing matched (None for None).  The call's DISTINCT stop
        sets are packed into one table (equal strings share states).  The buffers are the store's, one set per (row count,
        state capacity) with the capacity rounded up to a power of two: calls whose stop strings differ but need tables of
        similar size share the addresses and with them their captured chunks.  Stop strings need the bytes of every id
        (``_vocab_bytes``; uploaded once per vocabulary object); stop sets of ids alone need none."""
        if rows is None:
            return None
        distinct = list(dict.fromkeys(s for s in rows if s is not None))
        table = stops.pack(distinct)
        start = dict(zip(distinct, table.starts))
        trans, match_len, match_id, cap = stops.padded(table)
        b, ids_cap = len(rows), len(rows) * stops.STOP_IDS_MAX
        tok_off = tok_bytes = None
        vocab = n_bytes = 0
        if any(s.strings for s in distinct):
            tok_off, tok_bytes, n_bytes = self._vocab_on_device(self._vocab_bytes("stop", vocab_bytes))
            vocab = self.config.text.vocab_size
        d16, d32 = self._store.fixed("stop", (b, cap), lambda: (
            torch.empty(cap * 257, dtype=torch.int16, device=self._device),
            torch.empty(cap + (b + 1) + ids_cap + b + 6 * b, dtype=torch.int32, device=self._device)))
        host = np.zeros(d32.numel(), dtype=np.int32)
        h_mid, h_ptr, h_ids, h_base, h_words = np.split(host, np.cumsum([cap, b + 1, ids_cap, b]))
        h_mid[:] = match_id
        counts = [len(s.token_ids) if s is not None else 0 for s in rows]
        h_ptr[1:] = np.cumsum(counts)
        h_ids[:] = -1
        h_ids[: int(h_ptr[-1])] = [t for s in rows if s is not None for t in s.token_ids]
        h_base[:] = [len(s.strings) if s is not None else 0 for s in rows]
        words = h_words.reshape(6, b)
        words[0] = [start[s] if s is not None else stops.NO_STOP for s in rows]
        words[3], words[5] = -1, -1
        d16.copy_(self._h2d(torch.from_numpy(np.concatenate([trans.reshape(-1), match_len]).view(np.int16))))
        d32.copy_(self._h2d(torch.from_numpy(host)))
        d_trans, d_len = torch.split(d16, [cap * 256, cap])
        d_mid, d_ptr, d_ids, d_base, d_words = torch.split(d32, [cap, b + 1, ids_cap, b, 6 * b])
        return Stop(d_trans, d_len, d_mid, d_ptr, d_ids, d_base, tok_off, tok_bytes, vocab, n_bytes, d_words.view(6, b), cap)

    def _grammar_constraint(self, kind: str, value, vocab_bytes: Optional[Sequence[bytes]]) -> TokenAutomaton:
        tk, v = self.config.tokenizer, self.config.text.vocab_size
        vocab_bytes = self._vocab_bytes(kind, vocab_bytes)
        if kind == "regex":
            if not isinstance(value, str):
                raise ValueError(f"regex must be a str, not {value!r}")
            pattern, key = value, value
        else:
            pattern = grammar.json_schema_to_regex(value)
            key = json.dumps(value)
        hit = self._grammar_cache.get((kind, key, id(vocab_bytes)))
        if hit is not None and hit[0] is vocab_bytes:
            return hit[1]
        special = {tk.bos_id, tk.answer_id, tk.thinking_id, tk.coord_id, tk.size_id, tk.start_ground_points_id, tk.end_ground_id}
        a = grammar.compile_dfa(grammar.regex_to_dfa(pattern), vocab_bytes, tk.eos_id, sorted(i for i in special if 0 <= i < v),
                                self._device, f"the pattern {pattern[:60]!r}" if kind == "regex" else "the JSON schema")
        self._grammar_cache[(kind, key, id(vocab_bytes))] = (vocab_bytes, a)  # (the vocabulary is kept: its id stays its own)
        return a

    def _token_logprobs(self, logits: torch.Tensor, targets: torch.Tensor, suppress_id: int, logprob: torch.Tensor,
                        rank: torch.Tensor, suppress_rows: Optional[torch.Tensor] = None):
        """``logprob[r]`` (device fp32 [R]) and ``rank[r]`` (device int32 [R]) of token ``targets[r]`` (device int32 [R]) in row
        r of ``logits`` [R, V]: md_token_logprobs.  The log-probability is the model's own distribution at temperature 1,
        untruncated, with ``suppress_id`` left out in the rows ``suppress_rows`` marks (None: all of them; -1: in none) --
        not the tempered / top-p-renormalised distribution a sampled token was drawn from.  Rank 0: the row's argmax.
        Nothing is allocated and nothing synchronises: capturable."""
        r, v = logits.shape
        for t in (targets, logprob, rank) + ((suppress_rows,) if suppress_rows is not None else ()):
            assert t.is_contiguous() and t.numel() == r and t.device == logits.device
        assert targets.dtype == torch.int32 and rank.dtype == torch.int32 and logprob.dtype == torch.float32
        _lib.check(
            self.lib.md_token_logprobs(logits.data_ptr(), logits.stride(0), r, v, suppress_id,
                                       suppress_rows.data_ptr() if suppress_rows is not None else None, targets.data_ptr(),
                                       logprob.data_ptr(), rank.data_ptr(), self._stream()),
            "md_token_logprobs",
        )

    def _topk_logprobs(self, logits: torch.Tensor, gate: Optional[torch.Tensor], suppress_id: int, top_ids: torch.Tensor,
                       top_logprobs: torch.Tensor, suppress_rows: Optional[torch.Tensor] = None):
        """The k alternatives of every row of ``logits`` [R, V]: md_topk_logprobs.  ``top_ids`` (device int32 [R, k]) and
        ``top_logprobs`` (device fp32 [R, k]) take, at entry j, the live token of rank j and its log-probability -- the
        distribution, the suppression rule and the bits of ``_token_logprobs``.  ``gate`` (device int32 [R] or None): a row
        whose gate is no token id is not read and gets -1 / NaN (the step's tokens: idle rows).  Nothing is allocated and
        nothing synchronises: capturable."""
        r, v = logits.shape
        k = top_ids.shape[-1]
        for t in (top_ids, top_logprobs):
            assert t.is_contiguous() and t.shape == (r, k) and t.device == logits.device
        for t in (gate, suppress_rows):
            assert t is None or (t.is_contiguous() and t.numel() == r and t.dtype == torch.int32 and t.device == logits.device)
        assert top_ids.dtype == torch.int32 and top_logprobs.dtype == torch.float32
        _lib.check(
            self.lib.md_topk_logprobs(logits.data_ptr(), logits.stride(0), r, v, suppress_id,
                                      suppress_rows.data_ptr() if suppress_rows is not None else None,
                                      gate.data_ptr() if gate is not None else None, k, top_ids.data_ptr(),
                                      top_logprobs.data_ptr(), self._stream()),
            "md_topk_logprobs",
        )

    def _beam_select(self, logits: torch.Tensor, suppress_id: int, beam: Beam, beams_in: int, tokens_out: torch.Tensor,
                     parents_out: torch.Tensor):
        """One beam decision over ``logits`` (md_beam_select): [requests x num_beams, V], or, ``beams_in`` 1, the prompt
        pass's [requests, V].  The next beams' tokens go to ``tokens_out`` and their parents to ``parents_out`` (int32
        [requests x num_beams]); cum, pool, done flags and slot hand-off change in ``beam``'s arrays.  Nothing is allocated
        and nothing synchronises: capturable."""
        w = beam.num_beams
        rows = tokens_out.numel()
        assert logits.shape[0] * (w if beams_in == 1 else 1) >= rows and rows % w == 0 and parents_out.numel() == rows
        for t in (tokens_out, parents_out, beam.src, beam.dst, beam.frm, beam.to):
            assert t.is_contiguous() and t.dtype == torch.int32 and t.device == logits.device and t.numel() >= rows
        _lib.check(
            self.lib.md_beam_select(logits.data_ptr(), logits.stride(0), rows // w, w, beams_in, logits.shape[1], suppress_id, None,
                                    beam.eos_id, int(beam.early_stopping), C.byref(beam.state), tokens_out.data_ptr(),
                                    parents_out.data_ptr(), beam.src.data_ptr(), beam.dst.data_ptr(), beam.frm.data_ptr(),
                                    beam.to.data_ptr(), self._stream()),
            "md_beam_select",
        )

    def _kv_copy_tail(self, kv: _lib.MdKvCache, beam: Beam):
        """The KV tails of the beams ``_beam_select`` just chose, each to the slot its child decodes in, every layer
        (md_kv_copy_tail over the record's src / dst / from / to).  Capturable."""
        t = self.config.text
        _lib.check(
            self.lib.md_kv_copy_tail(C.byref(kv), t.n_layers, t.n_kv_heads, beam.n_slots, beam.src.numel(), beam.src.data_ptr(),
                                     beam.dst.data_ptr(), beam.frm.data_ptr(), beam.to.data_ptr(), self._stream()),
            "md_kv_copy_tail",
        )

    def _score(self, logits: torch.Tensor, targets: torch.Tensor, suppress_id: int, scores: Scores,
               gate: Optional[torch.Tensor] = None, suppress_rows: Optional[torch.Tensor] = None):
        """Fill ``scores`` (over [R]) for ``targets`` in ``logits`` [R, V]: ``_token_logprobs``, then ``_topk_logprobs`` if it has k."""
        self._token_logprobs(logits, targets, suppress_id, scores.logprob, scores.rank, suppress_rows=suppress_rows)
        if scores.k:
            self._topk_logprobs(logits, gate, suppress_id, scores.top_ids, scores.top_logprobs, suppress_rows=suppress_rows)

    def _first_token(self, logits: torch.Tensor, pick: Optional[Sampling] = None, row_perm=None,
                     uniforms: Optional[torch.Tensor] = None, scores: Optional[Scores] = None,
                     constraint: Optional[Constraint] = None, row0: int = 0) -> torch.Tensor:
        """The first generated token of every row, int32 [B], from its prompt pass's logits [B, V]: the argmax (``pick``
        None), a draw with the call's settings (``row_perm``: the draw order of these rows) or with each row's own (and
        ``uniforms`` fp32 [B]; a record with ``top_k`` / ``min_p`` is filtered like any later token).  Nothing is suppressed (moondream.py:313-318).  ``scores`` (a record over [B]): filled with
        the decision's log-probability, rank and alternatives, unsuppressed like the pick.  ``constraint``: these rows are
        rows ``row0 ..`` of the record -- the tokens their start states forbid lose their logits (in place) before the
        pick, and the scores are those of the masked logits."""
        if constraint is not None:
            assert not constraint.by_slot
            self._constrain(logits, None, _Rows(), constraint, row0)
        first = pick_tokens(self, pick, logits, -1, uniforms, row_perm=row_perm)
        if scores is not None:
            self._score(logits, first, -1, scores)
        return first

    # ---------------------------------------------------------- batched engine
    def _prefill_prompts(self, prompts: Sequence[Sequence[int]], pos: int, rows: Union[int, _Rows] = 0, prompt_embs=None,
                         last_only: bool = False):
        """Prefill B equal-length prompts at position ``pos``; returns (logits [B,V], hidden [B,T,D], pos+T).
        ``last_only``: for a caller that reads the logits alone -- hidden is [B,1,D], the last row of every sequence.
        reference: moondream.py:280-321 (per sequence)."""
        b = len(prompts)
        ids = torch.tensor(prompts, dtype=torch.int32)
        x = self._embed(ids) if prompt_embs is None else prompt_embs
        hidden = self._text_forward(x, pos, rows, keep="last" if last_only else "all")
        return self._lm_head(hidden), hidden, pos + ids.shape[1]

    def _decode_greedy(self, first: torch.Tensor, pos: Union[int, Sequence[int]], max_tokens: int, suppress_id: int,
                       rows: Union[int, _Rows] = 0, eos_id: Optional[int] = None, **kw):
        """``_decode_greedy_impl`` (``kw``: its further arguments) plus the safety net of the persistent single-sequence
        kernel: its software grid barriers need every workgroup resident; if one times out (the GPU was shared with another
        persistent kernel) the kernel raises an error word and finishes with garbage.  That state is fully re-initialised by
        decoding the same tokens again (K / V rows at positions >= ``pos``, the id history, the position buffer), so the call
        is repeated on the batched kernels and the persistent kernel is switched off for this model."""
        hist = self._decode_greedy_impl(first, pos, max_tokens, suppress_id, rows, eos_id, **kw)
        if self._b1_used:
            torch.cuda.current_stream(self._device).synchronize()
            if int(self._b1_sync[64 * 11]) != 0:
                import warnings

                with torch.inference_mode():
                    self._b1_sync[64 * 11] = 0
                self.single_sequence_kernel = False
                self._store.invalidate()
                warnings.warn("md_decode_step_b1: a grid barrier timed out (GPU shared with another persistent kernel?); "
                              "repeating the decode on the batched kernels and disabling the single-sequence kernel", RuntimeWarning)
                hist = self._decode_greedy_impl(first, pos, max_tokens, suppress_id, rows, eos_id, **{**kw, "allow_b1": False})
        return hist

    def _decode_greedy_impl(self, first: torch.Tensor, pos: Union[int, Sequence[int]], max_tokens: int, suppress_id: int,
                            rows: Union[int, _Rows] = 0, eos_id: Optional[int] = None, check_every: int = 16,
                            allow_b1: bool = True, sampling: Optional[Sampling] = None, scores: Optional[Scores] = None,
                            penalty: Optional[Penalty] = None, constraint: Optional[Constraint] = None,
                            stop: Optional[Stop] = None):
        """Device-resident decode loop: returns int32 [steps+1, B] (row 0 = ``first``).  ``sampling`` None: greedy.  Otherwise every
        step draws each sequence's token with the reference's rule (moondream.py:521-528: softmax(logits / T), _apply_top_p,
        multinomial) from the step's own logits on the device (md_sample_top_p), with one uniform per (step, sequence) taken
        UP FRONT from torch's generator -- no host round trip per token, replayable from a hipGraph -- and permuted by
        ``sampling.row_perm``, so that sampled rows in another order see the draws of the copy path.
        reference: the generator of moondream.py:471-530 without its per-token host sync.
        ``pos`` is the position of the next token, one int or one per sequence (sequences whose
        prompts differ in length decode in the same lockstep batch).
        The steps run in chunks (``run_chunk``): eagerly over the history itself, or with ``compile()`` replayed from a
        captured hipGraph over the fixed buffers of the chunk's shape.  ``rows``: the routing of every step (``_Rows``).
        ``scores``: a record over [>= max_tokens + 1, B] whose row 0 holds ``first``'s decision; the loop fills row i for the
        tokens of ``hist[i]`` (``_token_logprobs`` on the logits the step leaves, then ``_topk_logprobs`` when the record has
        alternatives: the launches after the step's pick, inside the captured graph) and changes no id for it.
        ``penalty``: the rows' penalty record (``_penalty_record``) -- every step extends the histories by the tokens it
        consumes (``first`` in its first step) and penalises its logits before the pick; the scores are then those of the
        penalised logits.  Such a call decodes on the batched kernels, never on the single-sequence one.
        ``constraint``: the rows' constraint record (``_constraint_record``), each row in the state ``first`` was picked
        under -- every step advances the states by the tokens it consumes and masks its logits before the pick
        (after the penalties); the scores are those of the masked logits.  Batched kernels only, like ``penalty``.
        ``stop``: the rows' stop record (``_stop_record``), nothing fed yet -- ``first`` goes through the matchers here, every
        later token inside its step (md_stop_rows after the pick), and the all-done check counts a row that has matched as
        done like one that has emitted its eos: one more small reduction at the same place, no further synchronisation.
        The loop cuts nothing: the result triples stay in ``stop.words`` for the caller.  Batched kernels only."""
        rows = _Rows.of(rows)
        b = first.shape[0]
        t = self.config.text
        for tab in (rows.slots, rows.variants):
            assert tab is None or tab.numel() == b
        self._ensure_batch(rows.span(b))
        pos_list = [int(pos)] * b if isinstance(pos, int) else [int(p) for p in pos]
        assert len(pos_list) == b
        max_tokens = max(0, min(max_tokens, t.max_context - 1 - max(pos_list)))
        hist = torch.zeros(max_tokens + 1, b, dtype=torch.int32, device=self._device)
        hist[0] = first
        self._b1_used = False
        if stop is not None:  # the prompt pass's token: the first one every matcher sees
            self._stop_rows(hist[0], rows, stop)
        if max_tokens == 0:
            return hist
        pos_base = self._h2d(torch.tensor(pos_list, dtype=torch.int32))
        uniforms = None
        if sampling is not None:
            uniforms = torch.rand(max_tokens, b, device=self._device, dtype=torch.float32, generator=sampling.generator)
            if sampling.row_perm is not None:
                uniforms = uniforms[:, sampling.row_perm].contiguous()
        pos_t = pos_base.clone()  # what eager steps advance
        if rows.lora is not None:
            # LoRA variant: the fused device-resident step has no side path; the same loop with the step from its pieces, eager,
            # still without a host sync per token.  Its pick (the argmax too) is a launch of its own, and a sampled one draws
            # AGAIN, per step, from the generator the unused ``uniforms`` above came from: odd, but these are the ids a sampled
            # LoRA call has always returned, and this loop keeps them.
            taken = 0

            def lora_step(tok_in):
                nonlocal taken
                if taken:
                    pos_t.add_(1)
                pos_h = [p + taken for p in pos_list]
                taken += 1
                return self._step_from_pieces(tok_in.reshape(b, 1), pos_h, rows, pos_dev=pos_t)[1]

            chunk = DecodeChunk(b, hist, pos_t, lambda i: rows, suppress_id, pick=sampling or Sampling(0.0, 0.0), step=lora_step,
                                penalty=penalty, constraint=constraint, stop=stop)
            # (a per-row record -- top_k / min_p -- has no per-step draw of its own: it keeps the uniforms taken up front)
            graphs, uniforms = False, uniforms if sampling is not None and sampling.per_row else None
        else:
            need = self._decode_ws_bytes(rows, b)
            # one sequence, greedy, plain contiguous routing: the whole step as ONE persistent launch (csrc/decode_b1.hip) when the
            # library says this model / cache / device fits its static limits and its grid can be co-resident; anything else
            # decodes on the batched kernels.  Never from the pipelined engine (allow_b1 = False): a second stream's persistent
            # GEMMs could keep workgroups of the grid off the chip and its software barriers would time out.
            b1 = (b == 1 and allow_b1 and sampling is None and penalty is None and constraint is None and stop is None
                  and self.single_sequence_kernel and rows.plain
                  and not bool(self.w.text.fp8)
                  and bool(self.lib.md_decode_step_b1_supported(C.byref(self.w.text), C.byref(self._kv_struct(rows.slot0)))))
            self._b1_used = b1
            if b1:
                if self._b1_sync is None:
                    self._b1_sync = torch.zeros(4096, dtype=torch.int32, device=self._device)
                need = max(need, self.lib.md_decode_step_b1_workspace_bytes(C.byref(self.w.text)))
            chunk = DecodeChunk(b, hist, pos_t, lambda i: rows, suppress_id, need, sampling, b1=b1, penalty=penalty,
                                constraint=constraint, stop=stop)
            graphs = self.use_graphs
        # one graph = `per` consecutive steps over fixed buffers; eager chunks end where the all-done check is due
        per = max(1, min(check_every or 16, max_tokens)) if graphs else (check_every or max_tokens)
        stream = torch.cuda.current_stream(self._device).cuda_stream if graphs else None
        steps = 0
        while steps < max_tokens:
            n = min(per, max_tokens - steps)
            into = scores and scores[steps + 1 :]  # where the steps leave their scores: in the record itself, or ...
            if graphs:
                # the fixed buffers of this shape on this stream (the pipelined engine's decode stream and the default stream
                # each have their own), refreshed before each replay; its graphs share them: a stream runs one chunk at a time
                zeros = lambda rows, dtype: torch.zeros(rows, b, dtype=dtype, device=self._device)
                buf, pos_buf, u_buf = self._store.fixed("chunk", (stream, b, n), lambda: (
                    zeros(n + 1, torch.int32), zeros(1, torch.int32)[0], zeros(n, torch.float32)))
                if scores is not None:  # ... in the fixed planes of this shape and k, which only a call that asks makes
                    into = self._store.fixed("chunk", (stream, b, n, "scores", scores.k), lambda: Scores.new((n, b), scores.k, self._device))
                buf[0] = hist[steps]
                pos_buf.copy_(pos_base + steps)
                if uniforms is not None:
                    u_buf.copy_(uniforms[steps : steps + n])
                part = replace(chunk, tokens=buf, pos=pos_buf, uniforms=u_buf if uniforms is not None else None)
            else:
                part = replace(chunk, tokens=hist[steps:], uniforms=uniforms[steps:] if uniforms is not None else None)
            run_chunk(self, replace(part, **into.chunk_fields()) if into else part, n, capture_stream=stream)
            if graphs:
                hist[steps + 1 : steps + n + 1] = buf[1:]
                if scores is not None:
                    scores[steps + 1 : steps + n + 1].copy_(into)
            steps += n
            if steps < max_tokens and stop is not None:  # a row is done at its eos or at its first stop match
                done = stop.at[:b] >= 0
                if eos_id is not None:
                    done = done | (hist[: steps + 1] == eos_id).any(dim=0)
                if bool(done.all()):
                    break
            elif steps < max_tokens and eos_id is not None and bool((hist[: steps + 1] == eos_id).any(dim=0).all()):
                break  # every sequence has emitted its EOS
        return hist[: steps + 1]

    def _replay_or_capture(self, key, body, may_capture=None) -> bool:
        return self._store.replay_or_capture(key, body, may_capture)

    def _check_b1_barriers(self):
        """Call after the tokens of a single-sequence decode have reached the host: the persistent kernel's grid barriers
        spin with a bound (they need every workgroup resident, which a second such kernel on another stream, or another
        process on the GPU, can prevent); a barrier that gave up raises the error word and the tokens are not valid."""
        if self._b1_sync is not None and int(self._b1_sync[64 * 11]) != 0:
            with torch.inference_mode():  # (the state tensor was created under inference mode)
                self._b1_sync[64 * 11] = 0
            raise _lib.MoondreamHipError(
                "md_decode_step_b1: a grid barrier timed out (the GPU was shared with another persistent kernel?); "
                "set single_sequence_kernel = False to decode on the batched kernels")

    def _decode_logits(self, b: int) -> torch.Tensor:
        return self._store.grow("logits", b, lambda: torch.empty(max(b, self._max_batch), self.config.text.vocab_size, dtype=BF16,
                                                                  device=self._device))

    @staticmethod
    def _truncate(seq: List[int], eos_id: Optional[int], max_tokens: int) -> List[int]:
        out = []
        for tok in seq:
            if (eos_id is not None and tok == eos_id) or len(out) >= max_tokens:
                break
            out.append(tok)
        return out

    def _prefill_groups(self, groups: Sequence[Tuple[int, int]], embed, pos: Union[int, Sequence[int]],
                        rows: Union[_Rows, Sequence[_Rows]], sampling: Optional[Sampling] = None,
                        logits_capture: Optional[torch.Tensor] = None, scores: Optional[Scores] = None, hidden_sink=None,
                        constraint: Optional[Constraint] = None, uniforms: Optional[torch.Tensor] = None,
                        head_rows: Optional[int] = None):
        """One decoder pass per group [r0, r1) of equal-length prompts: ``embed(r0, r1)`` [r1-r0, T, D] goes through the decoder
        at position ``pos`` (one int, or one per group) into the slots of ``rows.sub(r0, r1)`` (or of the group's own entry
        of ``rows``, one routing per group, already cut), then lm_head and the pick of the first token (``_first_token``;
        ``sampling`` None: argmax; a group draws in its rows' order among themselves in ``sampling.row_perm``; per-row
        settings, fp32 [B] like their ``uniforms``, are cut like the rows; without ``uniforms`` such rows draw from
        ``sampling.generator`` as the call's settings would).  ``head_rows``: lm_head, the pick and what goes
        with it run in cuts of at most so many rows of a pass (None: the whole pass).
        Returns (first int32 [B], hidden_last [B, D], next_pos list); the groups' logits go to ``logits_capture`` [B, V], each
        first decision's log-probability, rank and alternatives (unsuppressed, like the pick) to ``scores``, a record over [B].
        ``hidden_sink(r0, r1, hidden [r1-r0, T, D])``: the scorer's form -- every hidden row of the pass goes to the sink, and
        no first token is picked (``first`` and ``hidden_last`` are not filled).  ``constraint``: the rows' record, row r
        its entry r -- every first token is picked under its row's start state (``_first_token``)."""
        b = groups[-1][1]
        first = torch.empty(b, dtype=torch.int32, device=self._device)
        hidden_last = torch.empty(b, self.config.text.dim, dtype=BF16, device=self._device)
        next_pos = [0] * b
        pos_of = [pos] * len(groups) if isinstance(pos, int) else pos
        rows_of = [rows.sub(r0, r1) for r0, r1 in groups] if isinstance(rows, _Rows) else rows
        for (r0, r1), p, route in zip(groups, pos_of, rows_of):
            x = embed(r0, r1)
            next_pos[r0:r1] = [p + x.shape[1]] * (r1 - r0)
            if hidden_sink is not None:
                hidden_sink(r0, r1, self._text_forward(x, p, route, keep="all"))
                continue
            hidden = self._text_forward(x, p, route, keep="last")  # [r1-r0, 1, D]
            cut = head_rows or r1 - r0
            for c0 in range(r0, r1, cut):
                c1 = min(r1, c0 + cut)
                logits = self._lm_head(hidden[c0 - r0 : c1 - r0])
                if logits_capture is not None:
                    logits_capture[c0:c1] = logits
                perm = sampling.row_perm[c0:c1] if sampling is not None and sampling.row_perm is not None else None
                by_row = sampling is not None and sampling.per_row  # the rows' own settings and draws
                draws = uniforms[c0:c1] if uniforms is not None else None
                if by_row and draws is None:  # the call's generator: the draws ``_pick`` makes for these rows
                    draws = torch.rand(c1 - c0, device=self._device, dtype=torch.float32, generator=sampling.generator)
                    if perm is not None:
                        draws = draws[perm - perm.min()].contiguous()
                first[c0:c1] = self._first_token(logits, sampling.cut(c0, c1) if by_row else sampling,
                                                 perm - perm.min() if perm is not None else None, uniforms=draws,
                                                 scores=scores and scores[c0:c1], constraint=constraint, row0=c0)
            hidden_last[r0:r1] = hidden[:, -1, :]
        return first, hidden_last, next_pos

    def _place_images(self, images, rows: _Rows, mark, slots: Optional[Sequence[int]] = None) -> List[int]:
        """Image k's KV prefix into row k's slot of ``rows``: the raw images go through ONE ViT batch and every run of
        consecutive rows through one ``_prefill_images`` (which, like ``load_encoded_image``, also writes the slot's e4m3
        rows in the fp8 KV mode); EncodedImages are loaded -- into slot k, or, when ``rows`` has a slot table, into
        ``slots[k]``, its host copy.  Returns every image's prefix length."""
        raw = [k for k, im in enumerate(images) if not isinstance(im, EncodedImage)]
        for k in raw:
            if not isinstance(images[k], Image.Image):
                raise ValueError("image must be a PIL Image or EncodedImage")
        pos = [None] * len(images)
        if raw:
            img_emb = self._run_vision_encoder_batch([images[k] for k in raw], mark)
            mark("vision")
            for j0, j1 in _runs(raw):
                pos[raw[j0] : raw[j1 - 1] + 1] = [self._prefill_images(img_emb[j0:j1], rows.sub(raw[j0], raw[j1 - 1] + 1))] * (j1 - j0)
            mark("image_prefill")
        for k, im in enumerate(images):
            if isinstance(im, EncodedImage):
                self.load_encoded_image(im, k if slots is None else slots[k])
                pos[k] = im.pos
        return pos

    def _sequence_embeddings(self, prompts: Sequence[Sequence[int]], images=None, mark=None,
                             spatial: Optional[SpatialRecord] = None):
        """``embed(r0, r1)`` [r1-r0, T, D] for ``_prefill_groups`` over rows whose prompts are ``prompts``: the prompts'
        embeddings, for rows whose image prefix is in place -- or, with ``images`` (every row's own, all raw; ONE ViT
        batch, now), the fused prefill's rows.  There image prefix and prompt go through the decoder in ONE pass per group
        of equal-length prompts ([bos | 729 image embeddings | prompt] at position 0).  The attention kernels evaluate
        the reference's mask rule per element (bidirectional inside the first 730 positions, causal after), so this is
        the same computation as the reference's two passes (moondream.py:228-262 then 280-321) up to accumulation order
        -- one pass over the weights saved (fused_prefill = False keeps the two passes).
        ``spatial``: the rows' spatial references (moondream_amd/spatial.py), rows as in ``prompts``; its table goes to the
        device once, here, and every ``embed(r0, r1)`` stores the encoded references of rows [r0, r1) over their
        placeholder rows with one md_spatial_ref_embed launch -- no host synchronisation, no indexing by id.  None, or
        a record without tokens: the embeddings, and the launches, of the call without it."""
        embed_prompts = lambda r0, r1: self._embed(torch.tensor(prompts[r0:r1], dtype=torch.int32))
        if spatial is not None and not len(spatial):
            spatial = None
        if images is None:
            if spatial is None:
                return embed_prompts
            table = self._h2d(torch.from_numpy(spatial.table(0)))
            return lambda r0, r1: self._spatial_embed(embed_prompts(r0, r1), spatial, table, r0, r1, 0)
        img_emb = self._run_vision_encoder_batch(images, mark)
        if mark is not None:
            mark("vision")
        bos = self._embed(torch.full((len(images), 1), self.config.tokenizer.bos_id, dtype=torch.int32))
        fused = lambda r0, r1: torch.cat([bos[r0:r1], img_emb[r0:r1], embed_prompts(r0, r1)], dim=1)
        if spatial is None:
            return fused
        lead = 1 + img_emb.shape[1]
        table = self._h2d(torch.from_numpy(spatial.table(lead)))
        return lambda r0, r1: self._spatial_embed(fused(r0, r1), spatial, table, r0, r1, lead)

    def _spatial_embed(self, x: torch.Tensor, spatial: SpatialRecord, table: torch.Tensor, r0: int, r1: int, lead: int) -> torch.Tensor:
        """The spatial references of rows [r0, r1) encoded into ``x`` [r1-r0, T, D], those rows' embeddings ([bos | image
        | prompt] with ``lead`` positions in front of the prompt): ONE md_spatial_ref_embed launch over the rows'
        descriptors of ``table`` (``SpatialRecord.table(lead)`` on the device), none when they have no reference."""
        i0, i1 = spatial.span(r0, r1)
        if i1 == i0:
            return x
        assert x.is_contiguous() and x.dtype == BF16 and x.shape[0] == r1 - r0 and x.shape[1] == lead + spatial.prompt_len[r0]
        r, _ = self._region()
        ce, se = r["coord_encoder"], r["size_encoder"]
        d = x.shape[2]
        assert (ce.n, se.n, ce.k, se.k) == (d, d, 2 * r["coord_features"].shape[1], 2 * r["size_features"].shape[1])
        _lib.check(
            self.lib.md_spatial_ref_embed(table.data_ptr() + 16 * i0, i1 - i0, r["coord_features"].data_ptr(), ce.k, ce.w.data_ptr(),
                                          ce.k_pad, ce.b.data_ptr(), r["size_features"].data_ptr(), se.k, se.w.data_ptr(), se.k_pad,
                                          se.b.data_ptr(), d, x.data_ptr(), d, spatial.dst0_of(r0, lead), x.shape[0] * x.shape[1],
                                          self._stream()),
            "md_spatial_ref_embed",
        )
        return x

    def _shared_routing(self, plan: RowPlan, pos: int) -> _Rows:
        """The routing of a shared plan's rows over its prefix table (every prefix ``pos`` positions long), checked."""
        b = len(plan.order)
        check_shared_table(plan.own_slots, plan.prefix_slots, [pos] * b, [pos] * b, plan.n_slots)
        # one persistent buffer: captured decode graphs keep its addresses
        buf = self._store.grow("shared", 3 * b, lambda: torch.empty(3 * max(b, 64), dtype=torch.int32, device=self._device))
        buf[: 3 * b].copy_(self._h2d(torch.tensor(plan.own_slots + plan.prefix_slots + [pos] * b, dtype=torch.int32)))
        return _Rows(slots=buf[0:b], n_slots=plan.n_slots, prefix_slots=buf[b : 2 * b], prefix_len=buf[2 * b : 3 * b])

    def _prepare_sequences(self, images, prompts: Sequence[Sequence[int]], mark=None, rows: Union[int, _Rows] = 0,
                           fuse: bool = False, share_prefix: bool = False, variants: Optional[Sequence[int]] = None,
                           encode_settings: Optional[dict] = None, logits_capture: Optional[torch.Tensor] = None,
                           settings: Optional[CallSettings] = None, scores: Optional[Scores] = None, hidden_sink=None,
                           spatial: Optional[SpatialRecord] = None) -> Prepared:
        """Everything before the first generated token, for B (image, prompt-ids) pairs, as ``plan_rows`` lays them out
        (moondream_amd/shared_prefix.py): every image's KV prefix is placed (``_place_images``), then one prompt prefill per
        distinct length picks the first tokens.  Returns a ``Prepared``, rows in slot order.  The COPY route gives row r slot
        r under ``rows``, rows in stable order of prompt length.  The SHARED route (``share_prefix``, when ``_shares_prefix``
        and no ``variants``) places each distinct image (by identity) ONCE, into prefix slot k < P; the rows take slots P + r
        and read the prefix from there (md_text_forward_shared), and a sampled group draws in the copy route's row order
        (``row_perm``).  ``share_prefix`` that is not served shared runs the copy route over each distinct image's
        EncodedImage (``encode_settings``).  ``variants``: each row's bank index (-1: the base model) in the CALLER's order;
        the device table is built in slot order here.  ``fuse``: an all-raw copy route takes the one-pass prefill below.
        ``settings``: the call's settings record (moondream_amd/settings.py), rows in the CALLER's order; None: greedy, every
        row neutral.  Its three device records are built here, rows in slot order, and go to the decode loop in the
        ``Prepared``: the pick (a sampled call draws the first token as the reference's _prefill_prompt does,
        moondream.py:313-318, nothing suppressed there; with top-k / min-p through their per-row record,
        ``_filter_record``), the constraint (``_constraint_record``: it masks every first pick) and, once the prompt
        passes are queued, the penalties (``_penalty_record``: the first token is picked with an empty history).
        ``logits_capture`` / ``scores`` / ``hidden_sink``: as ``_prefill_groups`` takes them, in slot order.
        ``spatial``: the rows' spatial references in the CALLER's order (their placeholders are in ``prompts``, so rows
        group by their total length); reordered to slot order here and encoded into the prompt embeddings
        (``_sequence_embeddings``).  Must run under torch.inference_mode()."""
        mark = mark or (lambda name: None)
        rows = _Rows.of(rows)
        share = share_prefix and variants is None and self._shares_prefix(rows.lora)
        if any(len(p) == 0 for p in prompts):
            raise ValueError("empty prompt")
        if share_prefix and variants is None and not share:
            images = self._encode_distinct(images, encode_settings)
        plan = plan_rows(list(images), [len(p) for p in prompts], share)
        b = len(plan.order)
        self._select_kernels(b)
        prompts = [list(prompts[i]) for i in plan.order]
        st = settings.reorder(plan.order) if settings is not None else None  # rows in slot order
        sampling = Sampling(float(st.temperature), float(st.top_p), st.generator) if st is not None and st.temperature != 0 else None
        self._ensure_batch(plan.n_slots)
        if variants is not None:
            rows = _Rows(variants=self._variant_table([variants[i] for i in plan.order]), bank=self._bank)
        mark("start")
        fused = fuse and self.fused_prefill and not share and all(isinstance(im, Image.Image) for im in plan.placed)
        embed = self._sequence_embeddings(prompts, plan.placed if fused else None, mark,
                                          spatial=spatial.reorder(plan.order) if spatial is not None else None)
        pos = 0  # (fused: the one pass starts at the bos)
        if not fused:
            prefix = set(self._place_images(plan.placed, _Rows() if share else rows, mark))
            if len(prefix) > 1:
                raise ValueError("EncodedImage with a different prefix length than the rest of the batch")
            pos = prefix.pop()
            if share:
                rows = self._shared_routing(plan, pos)
                if sampling is not None:
                    sampling = replace(sampling, row_perm=torch.tensor(plan.copy_rank, dtype=torch.int64, device=self._device))
        constraint = self._constraint_record(st and st.constraints)
        sampling = self._filter_record(sampling, st and st.filters)
        out = self._prefill_groups(plan.groups, embed, pos, rows, sampling, logits_capture, scores=scores, hidden_sink=hidden_sink,
                                   constraint=constraint)
        if fused:  # the one pass is both
            mark("image_prefill")
        mark("prompt_prefill")
        stop_sets = st.stops if st is not None else None
        return Prepared(plan.order, *out, rows, sampling, constraint, self._penalty_record(st and st.penalties),
                        self._stop_record(stop_sets, st and st.stop_vocab_bytes), stop_sets)

    def _mark(self, marks: list, name: str):
        """Phase timing (``collect_timing``): an event on the current stream, named after the phase that ends there."""
        if self.collect_timing:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self._device))
            marks.append((name, e))

    def _phase_times(self, marks: list):
        """The time between consecutive marks of a call -> ``last_phase_ms``."""
        if self.collect_timing and len(marks) > 1:
            torch.cuda.synchronize(self._device)
            self.last_phase_ms = {marks[i][0]: marks[i - 1][1].elapsed_time(marks[i][1]) for i in range(1, len(marks))}

    def _shares_prefix(self, lora: Optional[PackedLora]) -> bool:
        """The shared-prefix path serves the base model, over the bf16 cache or (fp8 mode) its e4m3 copy; a LoRA variant
        takes the copy path (same results)."""
        return lora is None

    def _encode_distinct(self, images, settings: Optional[dict]) -> List[EncodedImage]:
        """Each distinct image object encoded once (``encode_image``), repeated per row: the copy path's input."""
        enc: Dict[int, EncodedImage] = {}
        for im in images:
            if id(im) not in enc:
                enc[id(im)] = self.encode_image(im, settings)
        return [enc[id(im)] for im in images]

    def batch_generate_ids(
        self,
        images: Sequence[Union[Image.Image, EncodedImage]],
        prompts: Sequence[Sequence[int]],
        max_tokens: int = DEFAULT_MAX_TOKENS,
        eos_id: Optional[int] = None,
        ignore_eos: bool = False,
        variant: Optional[str] = None,
        temperature: float = 0.0,
        top_p: float = DEFAULT_TOP_P,
        generator: Optional[torch.Generator] = None,
        share_prefix: bool = False,
        variants: Optional[Sequence[Optional[str]]] = None,
        return_logprobs: bool = False,
        top_logprobs: Optional[int] = None,
        repetition_penalty: Union[float, Sequence[float]] = 1.0,
        presence_penalty: Union[float, Sequence[float]] = 0.0,
        frequency_penalty: Union[float, Sequence[float]] = 0.0,
        constraints: Union[None, TokenAutomaton, Sequence[Optional[TokenAutomaton]]] = None,
        top_k: Union[int, Sequence[int]] = 0,
        min_p: Union[float, Sequence[float]] = 0.0,
        spatial: Optional[SpatialRecord] = None,
        stop=None,
        stop_token_ids=None,
        include_stop_str_in_output: bool = False,
        vocab_bytes: Optional[Sequence[bytes]] = None,
        return_finish: bool = False,
    ):
        """Token ids for B (image, prompt-ids) pairs, decoded in lockstep; greedy by default.

        ``share_prefix``: rows whose image is the same object (the same ``EncodedImage``, or the same PIL image by identity)
        read ONE copy of its KV prefix -- the image is encoded / loaded once, and the decode attention loads each prefix row
        once for a group of rows (md_decode_step_shared).  The ids are those of the same call with every image replaced by
        its ``EncodedImage`` (the copy path), greedy or sampled with the same ``generator`` seed, in the bf16 mode and in the
        fp8 KV mode (the decode steps then read one e4m3 prefix per image: csrc/attention_f8kv.hip).  A LoRA ``variant``
        takes the copy path.

        ``temperature`` > 0 (round 6): every sequence SAMPLES each of its tokens -- the first from the prompt pass's logits,
        the rest inside the lockstep loop -- with the reference's rule (softmax(logits / T), ``_apply_top_p``, multinomial:
        moondream.py:313-318, 521-528) on the device, one uniform per (step, sequence) from ``generator``; this is what the
        reference's loop of ``query`` / ``caption`` calls does at its DEFAULT settings (temperature 0.5, top_p 0.3:
        moondream.py:50-53; hf_moondream.py:99-103).  Sequences are statistically independent (own uniforms), not
        reproducible against torch.multinomial's stream.  The greedy contract below is the ``temperature = 0`` case.

        Defined as: element i is what the sequential path (encode_image ->
        load_encoded_image -> _generate_answer with temperature 0) returns for
        (images[i], prompts[i]).  Every BATCHED kernel's accumulation order is a
        function of the layer shape only, never of the number of sequences in
        the launch.  DEFAULT mode (round 4): ``batch_generate_ids(B)[i] ==
        batch_generate_ids([x_i])`` BIT FOR BIT whenever the lone sequence runs
        on the batched kernels (``single_sequence_kernel = False``): every launch
        of more than 64 rows takes the same four-wave GEMM whatever the batch
        (``_select_kernels``).  The one documented exception is the latency path
        of a lone sequence (``single_sequence_kernel`` on, the default: small
        tiles at prefill, the persistent kernel at decode), which agrees within
        bf16 accumulation-order noise.  ``caption`` / ``query`` on an
        ``EncodedImage`` make the reference's TWO decoder passes where a raw
        image takes one fused [image | prompt] pass here; equality with THAT
        path bit for bit is ``set_strict_batch_invariance(True)`` (two passes
        everywhere, priced in bench.py's ``strict_batch_invariance`` leg).
        Tested on the 64 unfiltered bench images at 2B.

        ``variants``: one LoRA variant per row (``None``: the base model), served in ONE batch -- every decode step streams
        the base weights once, and the grouped kernels of csrc/lora_multi.hip apply each row's low-rank pairs.  Each row's
        image prefix is prefilled under its own variant, as ``encode_image(image, settings={"variant": v})`` does.  Within
        such a call a row's ids do not depend on the other rows' variants.  A base row of a mixed call is not bit-identical
        to the same row in a base-only call: the mixed call rounds fc1's output to bf16 before GELU, as the reference does
        (layers.py:130-137), where the base path applies GELU in the GEMM epilogue in fp32.  Not with ``variant=``;
        ``share_prefix`` is ignored (copy path).

        ``return_logprobs``: returns ``(ids, logprobs, ranks)``; ``logprobs[i][j]`` and ``ranks[i][j]`` belong to ``ids[i][j]``
        and are truncated as the ids are.  A log-probability is log softmax of the logits the token was picked from, in the
        model's OWN distribution: temperature 1, untruncated, with ``answer_id`` left out from the second token on as generation
        leaves it out -- not the tempered / top-p-renormalised distribution a sampled token was drawn from.  ``ranks[i][j]``
        counts the tokens ahead of the pick in argmax order: 0 for every greedy token.  Computed on the device
        (md_token_logprobs: one launch after each step's pick, inside the captured chunk; one copy to the host at the end with
        the ids).  The flag changes no id; with it off the launches and captured graphs are unchanged.

        ``top_logprobs`` = k in 1 .. 32 (with ``return_logprobs``): returns ``(ids, logprobs, ranks, alternatives)``;
        ``alternatives[i][j]`` is a list of k ``(token_id, logprob)`` pairs, the k most probable live tokens of the decision
        that produced ``ids[i][j]`` in rank order (entry ``ranks[i][j]``, when below k, is the token itself with its own
        log-probability, bit for bit) -- the same distribution: the first decision unsuppressed, the later ones without
        ``answer_id``.  md_topk_logprobs: one more launch per step, after md_token_logprobs, in the same captured chunk;
        the same single copy to the host.  It changes no pick (this is not a top-k sampling rule); 0 / None: the call
        without it.  ValueError, before any GPU work: ``top_logprobs`` without ``return_logprobs``, or outside 1 .. 32.

        ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty``: one number, or one per row in the caller's
        order.  Before a token is picked, every token v the row has GENERATED so far (c times) has its logit x changed, in
        fp32: ``x = x / repetition_penalty if x > 0 else x * repetition_penalty`` (the HF / vLLM rule), then
        ``x -= presence_penalty + frequency_penalty * c`` (the OpenAI rule), rounded back to bf16 -- on the device
        (md_penalize_rows: one launch per step before the pick, inside the captured chunk; the histories live on the
        device).  The history is the generated tokens only: the first token, picked from the prompt pass's logits with
        an empty history, is in it, the prompt is not.  For ``repetition_penalty`` that differs from HF's processor,
        which also counts the prompt's tokens.  Sampling (``temperature``) draws from the penalised logits.  With
        ``return_logprobs`` the log-probabilities, ranks and alternatives are those of the PENALISED logits -- the
        distribution the token was picked from, before temperature and top-p -- so every greedy token still has rank 0.
        A row's ids depend on its own settings only; with every row neutral (1, 0, 0) the call is the one without the
        arguments, launch for launch.  Served in every mode of this call (``share_prefix``, ``variant``, ``variants``,
        the fp8 modes: a step leaves bf16 logits in the same buffer in all of them); a lone penalised sequence decodes on
        the batched kernels.  ValueError, before any GPU work: a repetition penalty that is not finite and > 0, a
        presence or frequency penalty that is not finite, a list that is not one per row.

        ``constraints``: one ``TokenAutomaton`` (moondream_amd/constraint.py) for every row, or a list with one entry per
        row in the caller's order (None: the row is free).  A row's automaton starts in state 0 and is advanced by every
        token the row generates; before each pick -- the first token's included -- the tokens its state forbids have
        their logits set to -inf on the device (md_constrain_rows: one launch per step after the penalties and before the
        pick, inside the captured chunk; the packed table and the rows' states live on the device), so neither the
        argmax nor a sampled draw can produce them.  A row that reaches ``FREE`` is unconstrained from there on.  With
        ``return_logprobs`` the log-probabilities, ranks and alternatives are those of the MASKED logits: a greedy token
        has rank 0 and an alternative outside the allowed set carries -inf.  A free row's ids are those of the call
        without the argument; with every row free the call is that call, launch for launch.  Served in every mode of
        this call, like the penalties; a lone constrained sequence decodes on the batched kernels.  ValueError, before
        any GPU work: a list that is not one per row, an entry that is no automaton, an automaton ``validate(vocab_size,
        answer_id)`` refuses (a state that allows no token other than ``answer_id``, which generation suppresses).

        ``top_k`` / ``min_p``: one value, or one per row in the caller's order -- two more truncation rules of a SAMPLED
        row, next to ``top_p``.  With the row's tokens in descending bf16 probability (ties by ascending id), ``top_k`` = k
        keeps the first k (0, or k >= the vocabulary: off) and ``min_p`` = m keeps the tokens of probability >=
        bf16(m * the best token's) (0: off; the best token always survives).  All three rules are judged on the SAME
        unrenormalised distribution and the shortest prefix survives, renormalised and drawn as before -- unlike HF / vLLM,
        which renormalise after top-k before top-p: here the cuts do not depend on an order, top-p stays the reference's
        bit for bit, and a row of (0, 0) is the row without the arguments.  On the device (md_sample_rows_filtered: the
        per-row pick, inside the captured chunk, the first token's included); they act after penalties and constraints,
        on the logits the pick reads.  A non-neutral value moves the call onto the per-row pick with the same draws; a
        greedy call (``temperature`` 0) accepts and ignores them; log-probabilities stay those of the unfiltered
        temperature-1 distribution.  A row's ids depend on its own settings only; with every row neutral the call is the
        one without the arguments, launch for launch.  Served in every mode of this call; a sampled LoRA ``variant`` call
        with them draws from the uniforms taken up front (as every other mode does), not per step.  ValueError, before
        any GPU work: a ``top_k`` that is not an integer >= 0, a ``min_p`` that is not finite or outside [0, 1], a list
        that is not one per row.

        ``spatial``: the rows' spatial references as a ``SpatialRecord`` (moondream_amd/spatial.py) in the caller's order,
        for prompts that hold their placeholders -- what ``batch_query(spatial_refs=)`` builds.  Each reference token is
        encoded on the device into its placeholder's row of the prompt embeddings (md_spatial_ref_embed: one launch per
        prompt pass, nothing else changes); None, or a record without tokens: the call without the argument.

        ``stop`` / ``stop_token_ids``: the caller's own end condition, matched on the device (md_stop_rows: one launch per
        step after the pick, inside the captured chunk; moondream_amd/stop.py).  ``stop``: one str, a list of str for
        every row, or a list with one entry per row (None, a str or a list of str; a list that holds a None or a list is
        read per row) -- up to 16 strings of 1 .. 64 bytes as UTF-8 per row.  ``stop_token_ids``: a list of ids for every
        row, or one list (or None) per row, up to 16.  A row's ids end at the EARLIEST of: its eos (excluded, as ever), a
        stop id (excluded like eos), the token in which a stop string completed -- INCLUDED, because a token cannot be
        split: the earliest end wins, and among the strings that end at that byte the longest is named.  (vLLM cuts the
        ids in front of that token when the string is excluded; here the ids keep it and ``Finish.text_bytes`` says where
        the text ends.)  Log-probabilities, ranks and alternatives are cut to the ids' length.  The loop's all-done check
        counts a matched row as done, so a call whose rows all stop early makes fewer steps.  Stop strings need the bytes
        every id spells: ``vocab_bytes`` (one bytes object per id), None: the model's tokenizer's, as ``regex_constraint``
        derives them; stop ids alone need none.  The launch reads token ids only: it changes no logit and no pick, a row
        without a stop set returns the ids of the call without the arguments, and with no row having one the call is
        that call, launch for launch.  Served in every mode of this call; a lone sequence with a stop set decodes on the
        batched kernels.  ``return_finish``: one more element is appended to the return value (``ids`` alone becomes
        ``(ids, finish)``): per row a ``Finish(reason, stop, text_bytes)`` -- "stop" / "eos" / "length", the matched string
        or id, and, when a string matched, the number of bytes of the ids' text that are the output (those in front of
        the string; with ``include_stop_str_in_output`` the string too).  ValueError, before any GPU work: an empty
        string, one of more than 64 bytes, more than 16 entries, an entry of the wrong type, an id outside the
        vocabulary, a per-row list of the wrong length, more than 4096 automaton states in all, and stop strings with
        the ``IdTokenizer`` stand-in and no ``vocab_bytes``.
        """
        if spatial is not None and spatial.n_rows != len(images):
            raise ValueError(f"spatial: a record of {spatial.n_rows} rows for {len(images)} rows")
        if temperature != 0:  # one value for the whole call (a list is a TypeError, as ever)
            temperature, top_p = float(temperature), float(top_p)
        st = CallSettings.of(len(images), self._check_automata, max_tokens=max_tokens,
                             temperature=temperature, top_p=top_p, generator=generator, variant=variant, variants=variants,
                             return_logprobs=return_logprobs, top_logprobs=top_logprobs, repetition_penalty=repetition_penalty,
                             presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, constraints=constraints,
                             top_k=top_k, min_p=min_p, stop=stop, stop_token_ids=stop_token_ids,
                             include_stop_str_in_output=include_stop_str_in_output, vocab_bytes=vocab_bytes,
                             vocab_size=None if stop is None and stop_token_ids is None else self.config.text.vocab_size)
        return self._generate_ids(images, prompts, st, eos_id, ignore_eos, share_prefix, return_logprobs, spatial, return_finish)

    def _generate_ids(self, images, prompts: Sequence[Sequence[int]], st: CallSettings, eos_id: Optional[int] = None,
                      ignore_eos: bool = False, share_prefix: bool = False, return_logprobs: bool = False,
                      spatial: Optional[SpatialRecord] = None, return_finish: bool = False):
        """``batch_generate_ids`` for a call whose settings are parsed: ``st`` is the call's settings record
        (moondream_amd/settings.py), one row per image; everything else as there."""
        if st.stops is not None and any(s is not None and s.strings for s in st.stops):
            self._vocab_bytes("stop", st.stop_vocab_bytes)  # (its errors: before any GPU work)
        b, max_tokens, variant, variants, top_k = len(images), st.max_tokens, st.variant, st.variants, st.top_logprobs
        assert b == len(prompts) and b > 0
        multi_rows = None
        if variants is not None:
            if variant is not None:
                raise ValueError("batch_generate_ids: variant= and variants= cannot be combined")
            if len(variants) != b:
                raise ValueError(f"variants has {len(variants)} entries for {b} rows")
            if any(v is not None for v in variants):
                if self._kv8_scales is not None or bool(self.w.text.fp8) or bool(self.w.text.f8):
                    raise ValueError("mixed LoRA variants are not served in the fp8 modes")
                multi_rows = [-1 if v is None else self._bank_index(v) for v in variants]
        tk = self.config.tokenizer
        eos = tk.eos_id if eos_id is None else eos_id
        marks: list = []
        mark = lambda name: self._mark(marks, name)
        lora = self._lora({"variant": variant})
        with torch.inference_mode():
            rows_t = max(0, min(max_tokens, self.config.text.max_context)) + 1  # row 0: the prefill's decision, then the loop's
            scores = Scores.new((rows_t, b), top_k, self._device, fill=True) if return_logprobs else None
            prep = self._prepare_sequences(images, prompts, mark, _Rows(lora=lora), fuse=True, share_prefix=share_prefix,
                                           variants=multi_rows, encode_settings={"variant": variant}, settings=st,
                                           scores=scores and scores[0], spatial=spatial)
            stop = None if ignore_eos else eos
            hist = self._decode_greedy(prep.first, prep.pos, max_tokens, tk.answer_id, prep.rows, stop, sampling=prep.sampling,
                                       scores=scores, penalty=prep.penalty, constraint=prep.constraint, stop=prep.stop)
            mark("decode")
            # the matchers' result triples travel with the history: ids [, triples], logprobs, ranks, alternatives in ONE copy
            ride = (hist,) if prep.stop is None else (hist, prep.stop.words[3:6, :b])
            host = scores and scores[: hist.shape[0]].to_host(*ride)
            if host:
                cols = host.extra[0].T.tolist()
                triples = host.extra[1].T.tolist() if prep.stop is not None else None
            elif prep.stop is not None:
                both = torch.cat([hist, ride[1]]).t().tolist()
                cols, triples = [c[:-3] for c in both], [c[-3:] for c in both]
            else:
                cols, triples = hist.t().tolist(), None
            if b == 1:
                self._check_b1_barriers()
            if triples is None and not return_finish:
                out = [[self._truncate(c, stop, max_tokens) for c in cols]]  # ids [, logprobs, ranks [, alternatives]] per slot
            else:  # the earliest of eos, a stop id (both excluded) and the token a stop string completed in (included)
                ends = []
                for r, c in enumerate(cols):
                    n_gen = min(len(c), max_tokens)
                    eos_at = c.index(stop, 0, n_gen) if stop is not None and stop in c[:n_gen] else None
                    at, keep, which = triples[r] if triples is not None else (-1, 0, -1)
                    ends.append(stops.finish_of(prep.stop_sets[r] if triples is not None else None, at, keep, which, n_gen,
                                                st.include_stop_str, eos_at))
                out = [[c[:n_ids] for c, (n_ids, _) in zip(cols, ends)]]
            n = [len(ids) for ids in out[0]]  # a leading run of the ids is kept: the same run of their values
            if return_logprobs:
                out += [[plane[: n[r], r].tolist() for r in range(b)] for plane in (host.logprob, host.rank)]
            if top_k:
                out.append([host.alternatives((slice(n[r]), r)) for r in range(b)])
            if return_finish:
                out.append([f for _, f in ends])
        self._phase_times(marks)
        out = tuple(prep.in_caller_order(per_row) for per_row in out)
        return out if return_logprobs or return_finish else out[0]

    BEAM_LOCKSTEP_ROWS = 128  # requests x num_beams one lockstep serves (the decode step's weight-stream regime); more: split

    def batch_beam_search_ids(self, images: Sequence[Union[Image.Image, EncodedImage]], prompts: Sequence[Sequence[int]],
                              num_beams: int, max_tokens: int = DEFAULT_MAX_TOKENS, eos_id: Optional[int] = None,
                              ignore_eos: bool = False, length_penalty: float = 1.0, early_stopping: bool = False,
                              num_return_sequences: int = 1) -> List[List[Hypothesis]]:
        """Beam search over B (image, prompt-ids) pairs: per request, in the caller's order, its ``num_return_sequences``
        best hypotheses, best first (``Hypothesis``: ``ids`` without the eos, ``score``, ``logprob``, ``finished``).

        A request keeps ``num_beams`` = W hypotheses (1 .. 16).  Each decision takes, per beam, the 2W most probable next
        tokens with their log-probabilities -- ``batch_generate_ids(top_logprobs=2W)``'s values bit for bit: temperature 1,
        ``answer_id`` live at the first decision and suppressed afterwards -- adds them to the beam's summed
        log-probability in fp32, and walks the 2W best of the W x 2W sums (ties: lower beam, then higher rank): an eos among
        the first W finishes a hypothesis, which enters the request's pool of W with score ``logprob * float32(1 /
        length ** length_penalty)`` (length counts the eos); an eos further down is dropped; the other candidates are the
        next W beams.  A request is done when its pool is full and ``early_stopping``, or its best beam's score at the
        current length cannot beat the pool's worst (HF's ``early_stopping=False`` rule).  At ``max_tokens`` every beam of a
        request that is not done enters the pool as an unfinished hypothesis under the same rule.  ``ignore_eos``: nothing
        finishes; every request runs to ``max_tokens``.  Beam rows are deterministic: there is no temperature / top-p / top-k
        / min-p here.

        On the device: each request's [image | prompt] is prefilled ONCE, into its own prefix slot, and its W
        beams decode as rows that read that prefix and keep only their tails in slots of their own
        (md_decode_step_shared).  After every step md_beam_select chooses the beams and md_kv_copy_tail moves each
        surviving tail to the slot its child reads -- both inside the captured chunk (``compile()``); the host reads the
        done flags once per chunk and the pools and planes once at the end.  The slab holds B x (1 + 2W) slots, sized up
        front; a call of more than ``BEAM_LOCKSTEP_ROWS`` beam rows is split by requests.  A request's result does not
        depend on the requests beside it wherever ``batch_generate_ids``' ids do not: bit for bit under
        ``set_strict_batch_invariance``.  In the default mode ONE request with ``single_sequence_kernel`` on has its
        prompt pass on the lone sequence's small-shape tiles, as ``batch_generate_ids([x])`` does, so its first decision
        can differ from the same request's in a batch within bf16 accumulation-order noise; its decode steps, W > 1 rows,
        run on the batched kernels with the pinned tiles either way.  The parent planes of the last call stay in
        ``last_beam_trace``.

        ValueError, before any GPU work: ``num_beams`` not an integer in 1 .. 16, ``num_return_sequences`` outside
        1 .. num_beams, a ``length_penalty`` that is not finite, an ``early_stopping`` that is not a bool, ``max_tokens`` < 1,
        an empty prompt, and the fp8 KV mode (the e4m3 copy of a moved tail is not kept; the fp8 / int4 WEIGHT streams are
        served: the step is unchanged)."""
        w, n_ret, lp, early = check_beams(num_beams, num_return_sequences, length_penalty, early_stopping)
        b = len(images)
        if b == 0 or b != len(prompts):
            raise ValueError(f"batch_beam_search_ids: {b} images and {len(prompts)} prompts")
        if any(len(p) == 0 for p in prompts):
            raise ValueError("empty prompt")
        if isinstance(max_tokens, bool) or int(max_tokens) < 1:
            raise ValueError(f"max_tokens must be an integer >= 1, not {max_tokens!r}")
        if self._kv8_scales is not None:
            raise ValueError("beam search is not served in the fp8 KV mode (the e4m3 copy of a moved KV tail is not kept)")
        eos = self.config.tokenizer.eos_id if eos_id is None else int(eos_id)
        per = max(1, self.BEAM_LOCKSTEP_ROWS // w)
        out: List[List[Hypothesis]] = []
        for r0 in range(0, b, per):
            out += self._beam_search(list(images[r0 : r0 + per]), [list(p) for p in prompts[r0 : r0 + per]], w, int(max_tokens),
                                     -1 if ignore_eos else eos, lp, early, n_ret)
        return out

    def _beam_buffers(self, stream, groups: int, w: int) -> dict:
        """The device arrays of a beam search over ``groups`` requests x ``w`` beams on ``stream``: made once per shape, so
        that a later call of the shape replays the graphs that bake their addresses in."""
        rows, dev = groups * w, self._device
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        return self._store.fixed("beam", (stream, groups, w), lambda: dict(
            cum=f32(rows), cur=i32(rows), own=i32(rows, 2), len=i32(groups), done=i32(groups), prefix_len=i32(groups),
            pool_n=i32(groups), pool_score=f32(groups, w), pool_sum=f32(groups, w), pool_parent=i32(groups, w),
            pool_step=i32(groups, w), inv_norm=f32(self.config.text.max_context + 2), cand_ids=i32(rows, 2 * w),
            cand_lp=f32(rows, 2 * w), src=i32(rows), dst=i32(rows), frm=i32(rows), to=i32(rows), prefix_slots=i32(rows),
            prefix_len_rows=i32(rows), pos=i32(rows)))

    def _beam_search(self, images, prompts, w: int, max_tokens: int, eos: int, length_penalty: float, early: bool,
                     n_ret: int, check_every: int = 16) -> List[List[Hypothesis]]:
        """``batch_beam_search_ids`` for requests that fit one lockstep (arguments checked; ``eos`` < 0: nothing finishes)."""
        g, t = len(images), self.config.text
        rows, n_slots = g * w, g * (1 + 2 * w)
        tk = self.config.tokenizer
        marks: list = []
        mark = lambda name: self._mark(marks, name)
        with torch.inference_mode():
            self._ensure_batch(n_slots)  # the whole call's slab, before anything is placed in it
            cap = torch.empty(g, t.vocab_size, dtype=BF16, device=self._device)
            # request r (slot order) is prefilled, [image | prompt], into slot r: its beams' shared prefix
            prep = self._prepare_sequences(images, prompts, mark, fuse=True, logits_capture=cap)
            prefix = [int(p) for p in prep.next_pos]
            # the steps run over requests x W rows: a lone request's beams are a batch, not the latency path of one
            # sequence (its prompt pass, above, ran as a lone sequence's does: see the docstring of the public call)
            self._select_kernels(rows)
            steps_max = min(max_tokens, t.max_context - 1 - max(prefix))
            if steps_max < 1:
                raise ValueError("beam search: the prompt leaves no room in the context")
            stream = torch.cuda.current_stream(self._device).cuda_stream
            buf = self._beam_buffers(stream if self.use_graphs else None, g, w)
            own = (g + 2 * np.arange(rows, dtype=np.int32)[:, None] + np.arange(2, dtype=np.int32)[None, :]).astype(np.int32)
            cum0 = np.full(rows, -np.inf, dtype=np.float32)
            cum0[::w] = 0.0
            inv_norm = inv_norm_table(t.max_context + 2, length_penalty)
            per_row = lambda xs: np.repeat(np.asarray(xs, dtype=np.int32), w)
            init = dict(cum=cum0, cur=own[:, 0], own=own, prefix_len=np.asarray(prefix, np.int32), inv_norm=inv_norm,
                        prefix_slots=per_row(range(g)), prefix_len_rows=per_row(prefix), pos=per_row(prefix))
            for name, arr in init.items():
                buf[name].copy_(self._h2d(torch.from_numpy(np.ascontiguousarray(arr))))
            for name in ("len", "done", "pool_n", "pool_score", "pool_sum", "pool_parent", "pool_step"):
                buf[name].zero_()
            for name in ("src", "dst"):
                buf[name].fill_(-1)
            state = _lib.MdBeamState(*(buf[n].data_ptr() for n in ("cum", "cur", "own", "len", "done", "prefix_len", "pool_n",
                                                                    "pool_score", "pool_sum", "pool_parent", "pool_step",
                                                                    "inv_norm")), inv_norm.size, buf["cand_ids"].data_ptr(),
                                     buf["cand_lp"].data_ptr())
            keep = tuple(buf[n] for n in ("cum", "cur", "own", "len", "done", "prefix_len", "pool_n", "pool_score", "pool_sum",
                                          "pool_parent", "pool_step", "inv_norm", "cand_ids", "cand_lp"))
            hist = torch.zeros(steps_max, rows, dtype=torch.int32, device=self._device)
            parents = torch.full((steps_max, rows), -1, dtype=torch.int32, device=self._device)
            beam = Beam(w, eos, early, state, parents, buf["src"], buf["dst"], buf["frm"], buf["to"], n_slots, keep)
            # decision 0, from the prompt pass's logits: one row per request, nothing suppressed, no tail to move yet
            self._beam_select(cap, -1, beam, 1, hist[0], parents[0])
            routing = _Rows(slots=buf["cur"], n_slots=n_slots, prefix_slots=buf["prefix_slots"], prefix_len=buf["prefix_len_rows"])
            chunk = DecodeChunk(rows, hist, buf["pos"], lambda i: routing, tk.answer_id, self._decode_ws_bytes(routing, rows),
                                beam=beam)
            graphs = self.use_graphs
            total = steps_max - 1  # decode steps: decision d >= 1 is step d - 1's
            per = max(1, min(check_every, total)) if graphs else check_every
            pos_base = buf["pos"].clone()
            steps = 0
            while steps < total:
                n = min(per, total - steps)
                if graphs:
                    tok_buf, par_buf = self._store.fixed("beam-chunk", (stream, g, w, n), lambda: (
                        torch.zeros(n + 1, rows, dtype=torch.int32, device=self._device),
                        torch.zeros(n, rows, dtype=torch.int32, device=self._device)))
                    tok_buf[0] = hist[steps]
                    buf["pos"].copy_(pos_base + steps)
                    part = replace(chunk, tokens=tok_buf, beam=replace(beam, parents=par_buf))
                else:
                    part = replace(chunk, tokens=hist[steps:], beam=replace(beam, parents=parents[steps + 1 :]))
                run_chunk(self, part, n, tag="beam", capture_stream=stream if graphs else None)
                if graphs:
                    hist[steps + 1 : steps + n + 1] = tok_buf[1:]
                    parents[steps + 1 : steps + n + 1] = par_buf
                steps += n
                if steps < total and bool(buf["done"].all()):  # the chunk's one host read
                    break
            mark("decode")
            host = {n: buf[n].cpu().numpy() for n in ("cum", "len", "done", "pool_n", "pool_score", "pool_sum", "pool_parent",
                                                      "pool_step")}
            toks = hist[: steps + 1].cpu().numpy().reshape(steps + 1, g, w)
            pars = parents[: steps + 1].cpu().numpy().reshape(steps + 1, g, w)
        self._phase_times(marks)
        self.last_beam_trace = {"tokens": toks[:, np.argsort(prep.order)], "parents": pars[:, np.argsort(prep.order)]}
        per_slot = [finalize(w, n_ret, int(host["len"][r]), bool(host["done"][r]), host["cum"][r * w : (r + 1) * w],
                             int(host["pool_n"][r]), host["pool_score"][r], host["pool_sum"][r], host["pool_parent"][r],
                             host["pool_step"][r], toks[:, r], pars[:, r], inv_norm) for r in range(g)]
        return prep.in_caller_order(per_slot)

    def _beam_best_ids(self, images, prompts: Sequence[Sequence[int]], settings: Optional[dict],
                       beams: Tuple[int, float, bool]) -> List[List[int]]:
        """The string API's beam route: the best hypothesis's ids per request.  ``settings``' ``max_tokens`` applies; what
        beam search does not serve is refused here, what it ignores (temperature, top_p, top_k, min_p: beam rows are
        deterministic) was checked with the call's settings and is unused."""
        st = settings or {}
        where = "beam search (num_beams > 1)"
        refuse_settings(settings, where, ("penalties", "constraints"), len(images))
        if st.get("variant") is not None or st.get("variants") is not None:
            raise ValueError(f"LoRA variant / variants are not served by {where}")
        w, lp, early = beams
        hyps = self.batch_beam_search_ids(images, prompts, w, max_tokens=st.get("max_tokens", DEFAULT_MAX_TOKENS),
                                          length_penalty=lp, early_stopping=early)
        return [h[0].ids for h in hyps]

    def _check_automata(self, constraints, n: int) -> Optional[List[Optional[TokenAutomaton]]]:
        """``check_constraints`` for this model: its vocabulary, and ``answer_id``, which generation suppresses."""
        return check_constraints(constraints, n, self.config.text.vocab_size, self.config.tokenizer.answer_id)

    def _settings_of(self, settings: Optional[dict], n: int) -> CallSettings:
        """The settings record of a string-API call over ``n`` rows (``CallSettings.of_settings``: every check, and last
        the compilation of a ``regex`` / ``json_schema``): made once, by the public call, before any other GPU work."""
        with_stops = settings is not None and (settings.get("stop") is not None or settings.get("stop_token_ids") is not None)
        return CallSettings.of_settings(settings, n, self._check_automata, self._grammar_constraint,
                                        self.config.text.vocab_size if with_stops else None)

    def _string_ids(self, images, prompts: Sequence[Sequence[int]], settings: Optional[dict], st: Optional[CallSettings] = None,
                    text: bool = False, **kw):
        """The ids behind ``batch_caption`` / ``batch_query`` / ``query_many``: ``_generate_ids`` with the record of
        ``settings`` (``st``: the caller has made it already; ``kw``: the call's further arguments), or, with
        ``settings["num_beams"]`` > 1, the best beam hypothesis.  ``text``: the rows' strings instead -- the tokenizer's
        decoding of the ids, except for a row that stopped on a stop STRING (``settings["stop"]``): that row returns the
        bytes of its ids cut to ``Finish.text_bytes``, decoded as UTF-8 with ``errors="replace"``."""
        st = st or self._settings_of(settings, len(images))
        if st.beams is not None:
            if kw.get("spatial") is not None:  # (beam rows are prepared by a route that takes no record)
                raise ValueError("num_beams > 1 (beam search) is not served with spatial_refs")
            ids = self._beam_best_ids(images, prompts, settings, st.beams)
        elif text and st.stops is not None:
            ids, ends = self._generate_ids(images, prompts, st, return_finish=True, **kw)
            spell = self._vocab_bytes("stop", st.stop_vocab_bytes) if any(f.text_bytes is not None for f in ends) else None
            return [self.tokenizer.decode(s) if f.text_bytes is None else
                    stops.cut_text([spell[t] for t in s], f).decode("utf-8", errors="replace") for s, f in zip(ids, ends)]
        else:
            ids = self._generate_ids(images, prompts, st, **kw)
        return [self.tokenizer.decode(s) for s in ids] if text else ids

    def batch_generate_ids_continuous(self, images, prompts: Sequence[Sequence[int]], max_tokens: Union[int, Sequence[int]] = DEFAULT_MAX_TOKENS,
                                      eos_id: Optional[int] = None, ignore_eos: bool = False, max_live: int = 64, chunk: int = 16,
                                      temperature: Union[float, Sequence[float]] = 0.0,
                                      top_p: Union[float, Sequence[float]] = DEFAULT_TOP_P, seeds=None,
                                      variant: Optional[str] = None, return_logprobs: bool = False,
                                      top_logprobs: Optional[int] = None, repetition_penalty=None, presence_penalty=None,
                                      frequency_penalty=None, constraints=None, top_k=None, min_p=None, stop=None,
                                      stop_token_ids=None, include_stop_str_in_output: bool = False, vocab_bytes=None,
                                      return_finish: bool = False, stop_states: Optional[int] = None):
        """``stop`` / ``stop_token_ids`` / ``include_stop_str_in_output`` / ``vocab_bytes`` / ``return_finish``:
        ``batch_generate_ids``' arguments, rule and return value per request; a request that matches gives its KV slot to
        the next queued one (``stop_states``: the engine's table size, None: its default).
        ``batch_generate_ids`` with continuous batching (moondream_amd/continuous.py): per-request ``max_tokens`` and EOS
        exit, freed KV slots refilled from the queue mid-decode; same greedy ids as the lockstep path.  ``temperature`` and
        ``top_p``: one float, or one per request (greedy and sampled requests share the decode steps).  ``return_logprobs``:
        (ids, logprobs, ranks) as ``batch_generate_ids`` returns them (``ContinuousEngine(logprobs=True)``); with
        ``top_logprobs`` = k also its ``alternatives`` (``ContinuousEngine(logprobs=True, top_logprobs=k)``).  The three
        penalties: one number or one per request (None: neutral), ``batch_generate_ids``' rule per request.  ``constraints``:
        one ``TokenAutomaton`` or one entry per request (None: free), ``batch_generate_ids``' rule and ids per request.
        ``top_k`` / ``min_p``: one value or one per request (None: off), ``batch_generate_ids``' rule per request."""
        from .continuous import ContinuousEngine

        eng = ContinuousEngine(self, max_live, chunk, logprobs=bool(return_logprobs), top_logprobs=top_logprobs,
                               **({} if stop_states is None else {"stop_states": stop_states}))
        return eng.generate(images, prompts, max_tokens, eos_id, ignore_eos, seeds, variant, temperature, top_p,
                            return_logprobs=bool(return_logprobs), repetition_penalty=repetition_penalty,
                            presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, constraints=constraints,
                            top_k=top_k, min_p=min_p, stop=stop, stop_token_ids=stop_token_ids,
                            include_stop_str_in_output=include_stop_str_in_output, vocab_bytes=vocab_bytes, return_finish=return_finish)

    def teacher_forced_logits(self, images, prompts: Sequence[Sequence[int]], forced_ids, gather_idx) -> torch.Tensor:
        """Parity instrument (tests / bench.py): the logits of every greedy decision when each sequence is FORCED to follow
        ``forced_ids[i]`` (the reference's ids) instead of its own argmax, gathered at ``gather_idx[i][j]`` (the reference's
        top-k ids of decision j).  Decision 0 is the prompt prefill's, decision j the decode step that consumed
        forced_ids[i][j-1] -- the same launches as ``batch_generate_ids`` at B > 1 (fused or two-pass prefill as configured, the
        batched decode step ``md_decode_step``), so the error measured here is the error of the ids' own logits.  At B = 1
        with ``single_sequence_kernel`` on, generation uses the persistent single-sequence kernel and this method still the
        batched one: it certifies batches, not that kernel (which tests/test_model_gpu.py compares separately).  Returns float32 [B, T+1, k] on the CPU (``answer_id`` suppressed from decision 1 on, moondream.py:517)."""
        b = len(images)
        forced = torch.as_tensor(np.asarray(forced_ids), dtype=torch.int32)
        idx = torch.as_tensor(np.asarray(gather_idx), dtype=torch.int64)
        t_steps = forced.shape[1]
        assert forced.shape[0] == b and idx.shape[0] == b and idx.shape[1] >= t_steps + 1
        tk, t = self.config.tokenizer, self.config.text
        out = torch.empty(b, t_steps + 1, idx.shape[2], dtype=torch.float32)
        with torch.inference_mode():
            cap = torch.empty(b, t.vocab_size, dtype=BF16, device=self._device)
            prep = self._prepare_sequences(images, prompts, fuse=True, logits_capture=cap)
            src = torch.tensor(prep.order, dtype=torch.int64)
            forced_s, idx_s = forced[src].to(self._device), idx[src].to(self._device)  # slot order
            vals = torch.empty(b, t_steps + 1, idx.shape[2], dtype=torch.float32, device=self._device)
            vals[:, 0] = torch.gather(cap.float(), 1, idx_s[:, 0])
            hist = torch.cat([forced_s.t().contiguous(), torch.zeros(1, b, dtype=torch.int32, device=self._device)], 0)
            scratch = torch.empty(b, dtype=torch.int32, device=self._device)
            logits = self._decode_logits(b)
            rows = prep.rows
            ws = self._workspace(self._decode_ws_bytes(rows, b), 2)
            kv = self._kv_struct(0)
            pos_t = torch.tensor([int(p) for p in prep.next_pos], dtype=torch.int32, device=self._device)
            for j in range(t_steps):
                self._decode_step(rows, hist[j], scratch, pos_t, b, tk.answer_id, logits, ws, kv)
                vals[:, j + 1] = torch.gather(logits[:b].float(), 1, idx_s[:, j + 1])
            out[src] = vals.cpu()
        return out

    # ------------------------------------------------------------- scoring
    def _check_score_args(self, images, prompts, continuations) -> None:
        """``score_ids``' argument checks: host data only, before any device work."""
        if self._kv8_scales is not None or bool(self.w.text.fp8) or bool(self.w.text.f8):
            raise ValueError("score_ids is not served in the fp8 modes")
        n = len(images)
        if n == 0 or len(prompts) != n or len(continuations) != n:
            raise ValueError(f"score_ids: {n} images, {len(prompts)} prompts and {len(continuations)} continuations")
        for i in range(n):
            if not isinstance(images[i], (EncodedImage, Image.Image)):
                raise ValueError("image must be a PIL Image or EncodedImage")
            if len(prompts[i]) == 0:
                raise ValueError(f"score_ids: empty prompt (row {i})")
            if len(continuations[i]) == 0:
                raise ValueError(f"score_ids: empty continuation (row {i})")
            prefix = images[i].pos if isinstance(images[i], EncodedImage) else 1 + self.config.vision.n_patches
            total = prefix + len(prompts[i]) + len(continuations[i])
            if total > self.config.text.max_context:
                raise ValueError(f"score_ids: image prefix + prompt + continuation ({total} positions, row {i}) do not fit the "
                                 f"{self.config.text.max_context}-slot context")

    def score_ids(self, images: Sequence[Union[Image.Image, EncodedImage]], prompts: Sequence[Sequence[int]],
                  continuations: Sequence[Sequence[int]], share_prefix: bool = False, variant: Optional[str] = None,
                  top_logprobs: Optional[int] = None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                  constraints=None, spatial_refs=None, stop=None, stop_token_ids=None):
        """Score GIVEN continuations: returns ``(logprobs, ranks)``, one list per row with one entry per token of
        ``continuations[i]`` -- the values ``batch_generate_ids(..., return_logprobs=True)`` attaches to a token it generates,
        for the tokens the caller supplies.  ``logprobs[i][j]`` is log softmax of the model's logits after
        (images[i], prompts[i], continuations[i][:j]) at continuations[i][j]: the model's OWN distribution at temperature 1,
        untruncated, with ``answer_id`` left out from the second token on as generation leaves it out -- not a tempered or
        top-p-renormalised one.  ``ranks[i][j]`` counts the tokens ahead of it in argmax order (0: greedy decoding picks it).

        No decode step runs: row i prefills ``prompts[i] + continuations[i][:-1]`` after its image prefix exactly as a prompt
        is prefilled (one pass per sequence length; ``share_prefix``: rows of the same image object read one copy of its
        prefix, bit-equal to the copy path; a LoRA ``variant`` takes the copy path), the hidden rows of the decisions are
        gathered compactly, lm_head runs over them in launches of <= 64 rows (the decode-regime kernels whatever the call's
        size: a row's values do not depend on what else is scored) and ONE md_token_logprobs launch reduces every row.  The
        KV slots used are scratch, as in any batch call.  ValueError, before any device work: an empty prompt or
        continuation, lists of different lengths, prefix + prompt + continuation beyond ``max_context``, the fp8 modes.

        ``top_logprobs`` = k in 1 .. 32: returns ``(logprobs, ranks, alternatives)``; ``alternatives[i][j]`` is the list of
        the k most probable live tokens of decision j as ``(token_id, logprob)`` pairs in rank order, as
        ``batch_generate_ids(..., top_logprobs=k)`` gives them: ONE md_topk_logprobs launch over the same logits and
        suppression table, and the same copy to the host.  ValueError for a k outside 1 .. 32.  The penalty arguments of
        ``batch_generate_ids`` are not served here (ValueError for a non-neutral one): the scorer makes no decode step, so
        there is no history to penalise from -- scores are the model's own.  ``constraints`` likewise (ValueError), and
        ``spatial_refs`` (ValueError: the scorer's prompts carry no encoded references)."""
        refuse_settings(dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                             constraints=constraints, stop=stop, stop_token_ids=stop_token_ids),
                        {"spatial_refs": "score_ids / query_choices (the scorer's prompts carry no encoded references)",
                         "constraints": "score_ids (no token is picked: scores are the model's own)",
                         "penalties": "score_ids (no decode step runs: scores are the model's own)",
                         "stops": "score_ids (no token is generated: the continuations are the caller's)"},
                        ("spatial_refs", "constraints", "penalties", "stops"), len(images), spatial_refs)
        top_k = check_top_logprobs(top_logprobs, True)
        self._check_score_args(images, prompts, continuations)
        conts = [[int(t) for t in c] for c in continuations]
        seqs = [[int(t) for t in p] + c[:-1] for p, c in zip(prompts, conts)]
        tk, d = self.config.tokenizer, self.config.text.dim
        lora = self._lora({"variant": variant})
        with torch.inference_mode():
            passes: list = []  # (r0, r1, hidden [r1-r0, T, D]) per prefill pass, rows in slot order
            sink = lambda r0, r1, h: passes.append((r0, r1, h))
            prep = self._prepare_sequences(images, seqs, rows=_Rows(lora=lora), fuse=True, share_prefix=share_prefix,
                                           encode_settings={"variant": variant}, hidden_sink=sink)
            # row (j, k) of the compact table: decision k of slot j, the hidden row at offset len(prompt) - 1 + k of its
            # sequence -- the last len(continuation) rows of the pass
            parts, targets, suppress, spans = [], [], [], []  # spans: each slot's rows of the table, in slot order
            for r0, r1, h in passes:
                t_len, idx = h.shape[1], []
                for j in range(r0, r1):
                    c = conts[prep.order[j]]
                    idx += [(j - r0) * t_len + t_len - len(c) + k for k in range(len(c))]
                    spans.append(slice(len(targets), len(targets) + len(c)))
                    targets += c
                    suppress += [0] + [1] * (len(c) - 1)  # decision 0 is the prompt pass's: unsuppressed (moondream.py:313-318)
                parts.append(h.reshape(-1, d).index_select(0, self._h2d(torch.tensor(idx, dtype=torch.int64))))
            hidden = torch.cat(parts).unsqueeze(1)  # [R, 1, D]
            r = hidden.shape[0]
            logits = torch.empty(r, self.config.text.vocab_size, dtype=BF16, device=self._device)
            for i0 in range(0, r, 64):
                self._lm_head(hidden[i0 : i0 + 64], out=logits[i0 : i0 + 64])
            tab = self._h2d(torch.tensor([targets, suppress], dtype=torch.int32))
            scores = Scores.new((r,), top_k, self._device)
            self._score(logits, tab[0], tk.answer_id, scores, suppress_rows=tab[1])
            host = scores.to_host()  # one copy to the host
        spans = prep.in_caller_order(spans)
        out = [host.logprob[s].tolist() for s in spans], [host.rank[s].tolist() for s in spans]
        return out + ([host.alternatives(s) for s in spans],) if top_k else out

    # ------------------------------------------------------ pipelined batches
    def _streams(self):
        st = getattr(self, "_pipe_streams", None)
        if st is None:
            prio = int(os.environ.get("MD_PIPE_DECODE_PRIORITY", "-1"))   # (A/B knob; -1 = high priority, the default)
            st = self._pipe_streams = (torch.cuda.Stream(device=self._device), torch.cuda.Stream(device=self._device, priority=prio))
        return st

    pipeline_streams = int(os.environ.get("MD_PIPE_STREAMS", "2"))  # 2: decode on its own (priority) stream; 1: encode and decode in order on one stream

    def batch_generate_ids_pipelined(self, batches, max_tokens: int = DEFAULT_MAX_TOKENS, ignore_eos: bool = False,
                                     repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, constraints=None,
                                     top_k=0, min_p=0.0, spatial_refs=None, stop=None, stop_token_ids=None):
        """Generator over an iterable of (images, prompt-id lists) batches; yields each batch's greedy ids in order, one
        decode group late (a group = two consecutive batches of <= 64 sequences decoded as ONE lockstep of <= 128 -- round 6,
        ``pair_decode`` -- or one batch).  Two HIP streams: the MFMA-bound encode (vision + prefill) of batch k+1 on one, the HBM-bound lockstep
        decode of batch k on a second, higher-priority one, over disjoint KV-slab slot groups and disjoint workspaces.

          * The two streams' kernels DO overlap on the GPU (profiles/r04_pipelined_engine_streams_ab.txt: 50-86 % of a
            decode kernel's time has a tile GEMM or prefill attention running beside it; each side runs slower, the step
            as a whole is 3 % shorter than with every kernel in order on one stream: 260.5 vs 269 ms on the same box --
            ``pipeline_streams = 1`` / MD_PIPE_STREAMS=1 is that one-stream engine).
          * The host tiling of batch k+1 (PIL resize + crop cutting, ~26 ms at B = 64) is started on the thread pool as
            soon as batch k's crops are cut, i.e. under batch k's GPU time.
          * The ids of batch k travel to pinned host memory behind its last decode step and are collected after batch
            k+1 has been queued; nothing touches the default stream and no host array is copied from pageable memory
            (either makes the host wait for the device).

        Per batch the result is identical to ``batch_generate_ids`` (same kernels, same order).  The penalty arguments of
        that call are not served here: ValueError for a non-neutral one; nor are ``constraints`` (ValueError), nor ``top_k`` /
        ``min_p`` (ValueError for a non-neutral one: the engine decodes greedily), nor ``spatial_refs`` (ValueError)."""
        refuse_settings(dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                             constraints=constraints, top_k=top_k, min_p=min_p, stop=stop, stop_token_ids=stop_token_ids),
                        {"spatial_refs": "the pipelined engine (its prefill arena embeds token ids alone)",
                         "stops": "the pipelined engine (its paired decode keeps no matcher states)",
                         "filters": "the pipelined engine (it decodes greedily: there is no sampled row to cut)",
                         "constraints": "the pipelined engine (its paired decode keeps no automaton states)",
                         "penalties": "the pipelined engine (its paired decode keeps no histories)"},
                        ("spatial_refs", "filters", "constraints", "penalties", "stops"), spatial_refs=spatial_refs)
        return self._pipelined_loop(batches, max_tokens, ignore_eos)

    # Round 6: the decode of TWO consecutive batches runs as one lockstep decode (<= 128 sequences) when the library takes that
    # many rows in one pass over the weights (md_decode_step: 65 .. 128 rows on the 128 x 64 weight-streaming tile, same bits as
    # two passes of 64): 2.07 instead of 2.46 ms per token and 64 sequences at 2B.  Each batch is still encoded on its own
    # (launches of 64 images: what BASELINE's batch=64 names), results are still yielded per batch and in order, one PAIR late.
    pair_decode = os.environ.get("MD_PIPE_PAIR", "1") not in ("0", "")

    def _pipelined_loop(self, batches, max_tokens, ignore_eos):
        it = iter(batches)
        cur = next(it, None)
        pending = []
        tk = self.config.tokenizer
        eos = tk.eos_id
        run_s, dec_s = self._streams()
        if self.pipeline_streams not in (2, 3):
            dec_s = run_s
        group = 0
        # the tiling started ahead is this generator's: drained when it ends, however it ends (a consumer that stops early)
        staged = self._staging.stage(list(cur[0]), self.vit_chunk_crops) if cur is not None else None
        try:
            while cur is not None:
                b = len(cur[0])
                pair = self.pair_decode and 2 * b <= 128 and not bool(self.w.text.fp8) and self._kv8_scales is None
                cap = 2 * b if pair else b            # slots of one group: two groups alternate (encode into one, decode from the other)
                self._ensure_batch(2 * cap)
                self._select_kernels(b)
                base = group * cap
                group ^= 1
                firsts, p1s, sizes = [], [], []
                with torch.inference_mode():
                    run_s.wait_stream(torch.cuda.current_stream(self._device))
                    while True:
                        images, prompts = cur
                        images = list(images)
                        nb = len(images)
                        assert nb == len(prompts) and nb > 0 and len({len(p) for p in prompts}) == 1
                        slot0 = base + sum(sizes)
                        nxt = next(it, None)
                        with torch.cuda.stream(run_s):
                            img_emb = self._run_vision_encoder_batch(images, staged=staged)
                            # this batch's crops are cut and queued for upload: the pool is free for the next batch's tiling
                            staged = self._staging.stage(list(nxt[0]), self.vit_chunk_crops) if nxt is not None else None
                            if self.fused_prefill:  # [bos | image | prompt] in one decoder pass, as in _prepare_sequences
                                # assembled in a PREALLOCATED arena (one per batch shape; stream-ordered reuse on run_s: the previous
                                # pass has read it before these copies run) instead of a fresh torch.cat per step; the BOS column is
                                # written once
                                n_img, n_pr = img_emb.shape[1], len(prompts[0])
                                x = self._prefill_arena(nb, 1 + n_img + n_pr, tk.bos_id)
                                x[:, 1 : 1 + n_img].copy_(img_emb)
                                x[:, 1 + n_img :].copy_(self._embed(torch.tensor(prompts, dtype=torch.int32)))
                                logits = self._lm_head(self._text_forward(x, 0, slot0, keep="last"))
                                p1 = x.shape[1]
                            else:
                                pos = self._prefill_images(img_emb, slot0)
                                logits, _, p1 = self._prefill_prompts(prompts, pos, slot0, last_only=True)
                            firsts.append(self._first_token(logits))
                        p1s.append(p1)
                        sizes.append(nb)
                        cur = nxt
                        if not pair or len(sizes) == 2 or cur is None or len(cur[0]) != b:
                            break
                    with torch.cuda.stream(run_s):
                        first = firsts[0] if len(firsts) == 1 else torch.cat(firsts)
                        if dec_s is not run_s:
                            ev = torch.cuda.Event()
                            ev.record(run_s)
                    with torch.cuda.stream(dec_s):
                        if dec_s is not run_s:
                            dec_s.wait_event(ev)
                            first.record_stream(dec_s)
                        pos1 = p1s[0] if len(set(p1s)) == 1 else [p for p, n in zip(p1s, sizes) for _ in range(n)]
                        hist = self._decode_greedy(first, pos1, max_tokens, tk.answer_id, base, None, check_every=16, allow_b1=False)
                        # ids -> PINNED host memory behind the last decode step (a ``.tolist()`` at collection time is a
                        # synchronous copy on the default stream: it waits for everything queued on the device)
                        if self.pipeline_streams == 3:  # measurement only: rounds 1-3's collection (synchronous copy on the default stream)
                            hist_host = hist
                        else:
                            hist_host = self._pinned_ids(tuple(hist.shape))   # recycled by _collect: no cudaHostAlloc per step
                            hist_host.copy_(hist, non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(dec_s)
                pending.append((hist_host, done, sizes))
                if len(pending) > 1:
                    yield from self._collect(pending.pop(0), None if ignore_eos else eos, max_tokens)
            while pending:
                yield from self._collect(pending.pop(0), None if ignore_eos else eos, max_tokens)
        finally:
            if staged is not None:
                staged.drain()

    def _prefill_arena(self, b: int, t: int, bos_id: int) -> torch.Tensor:
        """bf16 [b, t, D] buffer of the pipelined engine's fused prefill input, column 0 = the BOS embedding."""
        key = (b, t)
        arenas = self.__dict__.setdefault("_prefill_arenas", {})
        x = arenas.get(key)
        if x is None:
            if len(arenas) >= 4:   # a handful of batch shapes at most: do not hoard
                arenas.clear()
            x = arenas[key] = torch.empty(b, t, self.config.text.dim, dtype=BF16, device=self._device)
            x[:, :1].copy_(self._embed(torch.full((b, 1), bos_id, dtype=torch.int32)))
        return x

    def _pinned_ids(self, shape) -> torch.Tensor:
        """A pinned int32 host buffer for one step's ids, from a free list that ``_collect`` refills (a pinned allocation per
        step is a driver call and a page-locking of its own; review, round 5)."""
        free = self.__dict__.setdefault("_pinned_id_free", {}).setdefault(shape, [])
        if free:
            return free.pop()
        with torch.inference_mode(False):
            return torch.empty(shape, dtype=torch.int32, pin_memory=True)

    def _collect(self, item, eos, max_tokens):
        """One decoded group -> the id lists of its batches, in order (a generator: one item per batch)."""
        hist, done, sizes = item
        done.synchronize()
        cols = hist.t().tolist()
        if hist.device.type == "cpu" and hist.is_pinned():
            self.__dict__.setdefault("_pinned_id_free", {}).setdefault(tuple(hist.shape), []).append(hist)
        if sum(sizes) == 1:
            self._check_b1_barriers()
        i0 = 0
        for n in sizes:
            yield [self._truncate(cols[i], eos, max_tokens) for i in range(i0, i0 + n)]
            i0 += n

    def batch_caption(self, images, length: str = "normal", settings: Optional[dict] = None) -> List[str]:
        tpl = self.config.tokenizer.templates["caption"]
        if tpl is None:
            raise NotImplementedError("Model does not support captioning.")
        if length not in tpl:
            raise ValueError(f"Model does not support caption length '{length}'.")
        return self._string_ids(images, [tpl[length]] * len(images), settings, text=True)

    def _query_prompts(self, questions: Sequence[str]) -> List[List[int]]:
        """The prompt ids of ``batch_query`` / ``query_many``."""
        tpl = self.config.tokenizer.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        return [
            list(tpl["prefix"]) + list(self.tokenizer.encode(q).ids) + list(tpl["suffix"]) + list(tpl["suffix"])
            for q in questions
        ]

    def _query_prompts_spatial(self, images, questions: Sequence[str], spatial_refs, tail: Optional[Sequence[int]] = None):
        """``(prompts, record)`` of a batched query with ``spatial_refs`` (one entry per row, checked here before any GPU
        work: ``check_spatial_refs``): row i's prompt is ``query``'s, [prefix | placeholders | question | tail]
        (moondream.py:577-604), and ``record`` the ``SpatialRecord`` of every reference token in the caller's order --
        None when no row has a reference: the prompts are then those of the call without the argument.  ``tail`` None:
        the plain query's, [suffix | suffix]."""
        tk = self.config.tokenizer
        tpl = tk.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        tail = list(tpl["suffix"]) * 2 if tail is None else tail
        if len(images) != len(questions):
            raise ValueError("one question per image")
        q_ids = [list(self.tokenizer.encode(q).ids) for q in questions]
        rows = check_spatial_refs(spatial_refs, len(q_ids), [im is not None for im in images], q_ids, tk.coord_id, tk.size_id,
                                  getattr(self.w, "region", None) is not None)
        refs = rows or [[]] * len(q_ids)
        prompts = [spatial_prompt_ids(tpl["prefix"], r, q + list(tail), tk.coord_id, tk.size_id) for r, q in zip(refs, q_ids)]
        if rows is None:
            return prompts, None
        return prompts, SpatialRecord.build(rows, len(tpl["prefix"]), [len(p) for p in prompts])

    def batch_query(self, images, questions: Sequence[str], settings: Optional[dict] = None, reasoning: bool = False,
                    spatial_refs=None):
        """Answers for B (image, question) pairs in lockstep: a list of strings.
        ``reasoning=True``: a list of ``{"reasoning": {"text", "grounding"}, "answer": str}`` -- element i is what
        ``query(images[i], questions[i], reasoning=True, settings=settings)`` returns (reference: moondream.py:541-618), with
        the whole control flow on the device: one lockstep decode loop in which every row is reasoning, being fed the query
        suffix, answering or done (md_decode_step_reason).  ``settings``: ``temperature`` / ``top_p`` /
        ``max_tokens`` (defaults 0.5 / 0.3 / 768; ``max_tokens`` bounds the reasoning and the answer separately, as in the
        reference) and ``generator``.  At ``{"temperature": 0}`` the ids are the single-sequence path's (bit for bit under
        ``set_strict_batch_invariance``).  A sampled row draws one uniform per step, taken up front from the call's generator
        on the device (the step that feeds the suffix token consumes a draw like any other), where ``query`` draws per token:
        the same distribution per decision, other ids.  Not served, NotImplementedError: LoRA ``variant`` / ``variants``, the fp8
        modes, a query template whose suffix is not one token, a checkpoint without a region head.

        ``spatial_refs``: one entry per row -- None, an empty list, or a list of points ``(x, y)`` / boxes ``(x0, y0, x1,
        y1)`` -- placed in front of the row's question as ``query(image, question, spatial_refs=refs)`` places them
        (moondream.py:577-604): row i returns what that call returns, up to the rounding of the encoder's accumulation
        order.  Every reference token of the call is encoded and stored into its placeholder's row of the prompt
        embeddings on the device (md_spatial_ref_embed: one launch per prompt pass, no host synchronisation); rows group
        by their total prompt length, placeholders included, and only the prompt embeddings change: shared prefixes,
        ``variant`` / ``variants``, the fp8 modes, penalties, constraints, top-k / min-p and ``reasoning=True`` are served as
        they are.  A row without refs is the row of the call without the argument; with no row having any, so is the
        call, launch for launch.  (``settings["spatial_refs"]`` is read when the argument is absent.)  ValueError, before
        any GPU work: not one entry per row, an entry that is no list of 2- / 4-tuples of finite numbers, a row whose
        question's own tokens contain ``coord_id`` / ``size_id``, ``num_beams`` > 1; NotImplementedError: a checkpoint
        without a region head.  Ranges are not checked (the reference checks none)."""
        spatial_refs = refs_of(settings, spatial_refs)
        if reasoning:  # (what the reasoning route does not serve is refused there: ``_check_reasoning_served``)
            return self._reasoning_answers(self._batch_query_reasoning(images, questions, settings, share_prefix=False,
                                                                       spatial_refs=spatial_refs))
        if spatial_refs is None:
            return self._string_ids(images, self._query_prompts(questions), settings, text=True)
        return self._string_ids_spatial(images, settings, self._query_prompts_spatial(images, questions, spatial_refs), text=True)

    def _string_ids_spatial(self, images, settings: Optional[dict], built, **kw):
        """``_string_ids`` of a query with ``spatial_refs``: ``built`` = ``_query_prompts_spatial``'s (prompts, record);
        beam search is not served with references (ValueError, before any GPU work: ``_string_ids``)."""
        prompts, spatial = built
        return self._string_ids(images, prompts, settings, **kw, **({"spatial": spatial} if spatial is not None else {}))

    def batch_generate(self, images, prompts: Optional[Sequence[str]] = None, settings: Optional[dict] = None) -> List[str]:
        """BASELINE.json's ``batch_generate``: captions when ``prompts`` is None, else answers, with the reference's sampling
        settings (``settings``: max_tokens / temperature / top_p / variant; defaults 768 / 0.5 / 0.3 as moondream.py:50-53).
        At ``{"temperature": 0}`` element i == caption(images[i]) / query(images[i], prompts[i]): bit for bit under
        ``set_strict_batch_invariance``, within bf16 accumulation-order noise otherwise -- see ``batch_generate_ids``."""
        if prompts is None:
            return self.batch_caption(images, "normal", settings)
        return self.batch_query(images, prompts, settings)

    # ------------------------------------------------------- sequential API
    def _prefill_prompt(self, prompt_tokens: torch.Tensor, pos: int, temperature: float, top_p: float,
                        spatial_refs: Optional[SpatialRefs] = None, attn_mask=None, lora=None, causal: bool = False,
                        constraint: Optional[Constraint] = None, filt: Optional[Sampling] = None):
        """reference: moondream.py:280-321.  ``constraint``: the sequence's record, masking the first pick.  ``filt``: the
        sequence's one-row record with ``top_k`` / ``min_p`` (``_filter_record``), cutting the first pick.  ``causal`` stands for the reference's
        ``attn_mask`` argument: the only non-default mask it ever passes is the plain
        lower-triangular one of a text-only query (moondream.py:571-575)."""
        self._select_kernels(1)  # a lone sequence's own tile policy, whatever an earlier (batch) call left in the structs
        with torch.inference_mode():
            ids = prompt_tokens.to(torch.int32)
            emb = self._embed(ids)
            if spatial_refs:
                enc = self.encode_spatial_refs(spatial_refs)
                emb[ids.to(self._device) == self.config.tokenizer.coord_id] = enc["coords"]
                if enc["sizes"] is not None:
                    emb[ids.to(self._device) == self.config.tokenizer.size_id] = enc["sizes"]
            hidden = self._text_forward(emb, pos, _Rows(lora=lora if isinstance(lora, PackedLora) else None), causal=causal)
            logits = self._lm_head(hidden)
            if filt is not None:  # the draw ``_pick`` makes, through the per-row pick
                nxt = self._first_token(logits, filt, uniforms=torch.rand(1, device=self._device, dtype=torch.float32),
                                        constraint=constraint)
            else:
                nxt = self._first_token(logits, Sampling(temperature, top_p) if temperature != 0 else None, constraint=constraint)
        return logits, hidden, nxt.reshape(1, 1), pos + ids.shape[1]

    def _generate_answer(self, prompt_tokens: torch.Tensor, pos: int, settings: Optional[dict] = None,
                         spatial_refs: Optional[SpatialRefs] = None, eos_id: Optional[int] = None, attn_mask=None,
                         causal: bool = False):
        """Generator of text pieces.  reference: moondream.py:434-539.  ``settings``: the call's settings record with one
        row (``caption`` / ``query`` have made it), or, as the reference's own callers give it, the dict it is made from.
        The penalties (``batch_generate_ids``' rule, over this sequence's generated tokens) act on every step's logits
        before its pick, in the chunked greedy loop and in the per-token sampled one alike; the constraint masks every
        pick, the first included; with ``top_k`` / ``min_p`` a sampled answer's picks, the first included, go through the
        per-row pick with one row."""
        st = settings if isinstance(settings, CallSettings) else self._settings_of(settings, 1)
        if st.stops is not None:
            raise ValueError("stop / stop_token_ids are not served by the single-sequence generator (caption / query route them "
                             "to the batched loop)")
        max_tokens, temperature, top_p = st.max_tokens, st.temperature, st.top_p
        penalties, filters, automata = st.penalties, st.filters, st.constraints
        lora = self._lora({"variant": st.variant})
        rows = _Rows(lora=lora)
        eos = eos_id if eos_id is not None else self.config.tokenizer.eos_id
        # decode steps attend to keys [0, pos] only, which both masks allow: the mask matters for the prompt
        with torch.inference_mode():
            constraint = self._constraint_record(automata)  # one state over the whole answer, at its start now
            filt = self._filter_record(Sampling(float(temperature), float(top_p)), filters) if filters and temperature != 0 else None
        pick = filt or (Sampling(temperature, top_p) if temperature != 0 else None)  # of every token after the first
        _, _, nxt, pos = self._prefill_prompt(prompt_tokens, pos, temperature, top_p, spatial_refs, attn_mask, lora=lora, causal=causal,
                                              constraint=constraint, filt=filt)

        def token_source():
            with torch.inference_mode():
                penalty = self._penalty_record(penalties)  # one history over the whole answer, empty now
            if temperature == 0 and lora is None:
                done = 0
                first = nxt.reshape(1).to(torch.int32)
                cur_pos = pos
                while done < max_tokens:
                    chunk = min(16, max_tokens - done)
                    hist = self._decode_greedy(first, cur_pos, chunk, self.config.tokenizer.answer_id, 0, None, penalty=penalty,
                                               constraint=constraint)
                    toks = hist[:, 0].tolist()
                    self._check_b1_barriers()
                    for tok in toks[:-1]:
                        yield tok
                    done += len(toks) - 1
                    cur_pos += len(toks) - 1
                    first = hist[-1]
                    if len(toks) - 1 < chunk:
                        break
                yield int(first[0])
            else:
                tok = nxt.reshape(1).to(torch.int32)
                cur_pos = pos
                while True:
                    yield int(tok[0])
                    if cur_pos >= self.config.text.max_context:  # context full: same bound as the greedy loop
                        return
                    with torch.inference_mode():
                        _, logits = self._step_from_pieces(tok.reshape(1, 1), cur_pos, rows)
                        cur_pos += 1
                        if penalty is not None:
                            self._penalize(logits, tok, rows, penalty)
                        if constraint is not None:
                            self._constrain(logits, tok, rows, constraint)
                        # moondream.py:517.  The call's settings draw inside ``_pick``, per step; a one-row record likewise,
                        # here: these are the ids a sampled answer has always had
                        tok = pick_tokens(self, pick, logits, self.config.tokenizer.answer_id,
                                          torch.rand(1, device=self._device, dtype=torch.float32) if filt is not None else None)

        def generator():
            # streaming detokeniser: flush on newline, CJK, or up to the last space
            # (reference: moondream.py:477-537)
            cache: List[int] = []
            print_len = 0
            n = 0
            for tok in token_source():
                if tok == eos or n >= max_tokens:
                    break
                n += 1
                cache.append(tok)
                text = self.tokenizer.decode(cache)
                if text.endswith("\n"):
                    piece, cache, print_len = text[print_len:], [], 0
                    if piece:
                        yield piece
                elif len(text) > 0 and _is_cjk_char(ord(text[-1])):
                    piece = text[print_len:]
                    print_len += len(piece)
                    if piece:
                        yield piece
                else:
                    sp = text.rfind(" ", print_len)
                    if sp >= print_len:
                        piece = text[print_len : sp + 1]
                        print_len += len(piece)
                        if piece:
                            yield piece
            if cache:
                piece = self.tokenizer.decode(cache)[print_len:]
                if piece:
                    yield piece

        return generator()

    def caption(self, image, length: Literal["normal", "short", "long"] = "normal", stream: bool = False,
                settings: Optional[dict] = None):
        """reference: moondream.py:625-651.  ``settings`` may carry ``repetition_penalty`` / ``presence_penalty`` /
        ``frequency_penalty`` (an extension: ``batch_generate_ids``' rule over the caption's generated tokens) and
        ``constraints`` (one ``TokenAutomaton``)."""
        st = self._settings_of(settings, 1)  # every check of the settings: before any other GPU work
        beams = st.beams
        tpl = self.config.tokenizer.templates["caption"]
        if tpl is None:
            raise NotImplementedError("Model does not support captioning.")
        if length not in tpl:
            raise ValueError(f"Model does not support caption length '{length}'.")
        if beams is not None:  # beam search: the batched route's best hypothesis, as one string
            if stream:
                raise ValueError("num_beams > 1 (beam search) is not served with stream=True")
            return {"caption": self.batch_caption([image], length, settings)[0]}
        if st.stops is not None:  # stop strings / ids: the batched route with one row (its loop carries the matcher)
            if stream:
                raise ValueError("stop / stop_token_ids are not served with stream=True")
            return {"caption": self.batch_caption([image], length, settings)[0]}
        enc = self.encode_image(image, settings)
        self.load_encoded_image(enc)
        prompt = torch.tensor([tpl[length]])
        gen = self._generate_answer(prompt, enc.pos, st)
        return {"caption": gen} if stream else {"caption": "".join(list(gen))}

    def query(self, image=None, question: str = None, reasoning: bool = False,
              spatial_refs: Optional[SpatialRefs] = None, stream: bool = False, settings: Optional[dict] = None):
        """reference: moondream.py:541-618, including the ``reasoning`` branch (thinking token -> _generate_reasoning
        -> answer after a second suffix).  ``settings`` may carry the penalty settings and ``constraints`` as ``caption``'s
        may; not with ``reasoning`` (ValueError)."""
        st = self._settings_of(settings, 1)  # every check of the settings: before any other GPU work
        tpl = self.config.tokenizer.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        if question is None:
            raise ValueError("question must be provided.")
        if spatial_refs and image is None:
            raise ValueError("spatial_refs can only be used with an image.")
        if st.beams is not None:  # beam search: the batched route's best hypothesis, as one string
            if reasoning or stream:
                raise ValueError("num_beams > 1 (beam search) is not served with reasoning=True or stream=True")
            if image is None or spatial_refs:
                raise ValueError("num_beams > 1 (beam search) is served for a query about an image, without spatial_refs")
            return {"answer": self.batch_query([image], [question], settings)[0]}
        if reasoning:
            self._refuse_for_reasoning(settings)
        if st.stops is not None:  # stop strings / ids: the batched route with one row (its loop carries the matcher)
            if stream:
                raise ValueError("stop / stop_token_ids are not served with stream=True")
            if image is None:
                raise ValueError("stop / stop_token_ids are served for a query about an image")
            return {"answer": self.batch_query([image], [question], settings, spatial_refs=[spatial_refs] if spatial_refs else None)[0]}
        if image is not None:
            enc = self.encode_image(image, settings)
            self.load_encoded_image(enc)
            pos, head, causal = enc.pos, list(tpl["prefix"]), False
        else:
            # text only: BOS + prefix at position 0 under the plain causal mask (moondream.py:564-575);
            # stale K/V beyond the positions written here are never read (kv_len bounds every kernel)
            self._ensure_batch(1)
            pos, head, causal = 0, [self.config.tokenizer.bos_id] + list(tpl["prefix"]), True
        spatial = []
        if spatial_refs:
            tk = self.config.tokenizer
            for ref in spatial_refs:
                spatial.extend([tk.coord_id, tk.coord_id] if len(ref) == 2 else [tk.coord_id, tk.coord_id, tk.size_id])
        prompt = head + spatial + list(self.tokenizer.encode(question).ids) + list(tpl["suffix"])
        extra = {}
        if reasoning:
            # moondream.py:593-603: [.., suffix, thinking] -> reasoning text until answer_id, then the answer after [suffix]
            prompt = prompt + [self.config.tokenizer.thinking_id]
            pos, text, grounding = self._generate_reasoning(torch.tensor([prompt]), pos, settings, spatial_refs, causal=causal)
            extra = {"reasoning": {"text": text, "grounding": grounding}}
            gen = self._generate_answer(torch.tensor([list(tpl["suffix"])]), pos, st, None, causal=causal)
        else:
            prompt = prompt + list(tpl["suffix"])
            gen = self._generate_answer(torch.tensor([prompt]), pos, st, spatial_refs, causal=causal)
        return {**extra, "answer": gen} if stream else {**extra, "answer": "".join(list(gen))}

    def _generate_reasoning(self, prompt_tokens: torch.Tensor, pos: int, settings: Optional[dict] = None,
                            spatial_refs: Optional[SpatialRefs] = None, attn_mask=None, causal: bool = False):
        """reference: moondream.py:323-432.  Generates the reasoning text (stops at ``answer_id``; ``eos`` and
        ``size`` tokens suppressed), grounding every ``coord`` token through the region head: the token's
        coordinate is decoded from the hidden state that predicted it and fed back as the next embedding.
        Returns (pos, text, grounding).  One host decision per token, like the reference."""
        settings = settings or {}
        max_tokens = settings.get("max_tokens", DEFAULT_MAX_TOKENS)
        temperature = settings.get("temperature", DEFAULT_TEMPERATURE)
        top_p = settings.get("top_p", DEFAULT_TOP_P)
        lora = self._lora(settings)
        rows = _Rows(lora=lora)
        tk = self.config.tokenizer
        _, hidden, nxt, pos = self._prefill_prompt(prompt_tokens, pos, temperature, top_p, spatial_refs, attn_mask, lora=lora, causal=causal)
        last_hidden = hidden[:, -1:, :].reshape(1, -1)
        text_chunks: List[List[int]] = [[]]
        grounding_chunks: List[List[float]] = [[]]
        generated = 0
        bins = torch.zeros(1, 1, dtype=torch.int32, device=self._device)
        n_bins = self.config.region.coord_out_dim
        suppress = torch.tensor([tk.eos_id, tk.size_id], device=self._device)
        with torch.inference_mode():
            tok = int(nxt.reshape(-1)[0])
            while tok != tk.answer_id and generated < max_tokens and pos < self.config.text.max_context:
                if tok in (tk.start_ground_points_id, tk.end_ground_id):
                    text_chunks.append([])
                    grounding_chunks.append([])
                text_chunks[-1].append(tok)
                if tok == tk.coord_id:
                    # coordinate bin from the hidden state, value fed back through the coordinate encoder (device resident)
                    x = self._region_pick_encode(last_hidden, "coord", bins).reshape(1, 1, -1)
                    grounding_chunks[-1].append((bins[0, 0].to(torch.int64) / n_bins).item())
                else:
                    x = torch.tensor([[tok]])
                h, logits = self._step_from_pieces(x, pos, rows)
                logits[:, suppress] = float("-inf")  # moondream.py:397-398
                pos += 1
                last_hidden = h.reshape(1, -1)
                tok = int(self._pick(logits, temperature, top_p)[0])
                generated += 1
        texts = [self.tokenizer.decode(c) for c in text_chunks]
        grounding, start = [], 0
        for t, g in zip(texts, grounding_chunks):
            if len(g) > 1:
                pts = [(g[i], g[i + 1]) for i in range(0, len(g) - (len(g) % 2), 2)]
                grounding.append({"start_idx": start, "end_idx": start + len(t), "points": pts})
            start += len(t)
        return pos, "".join(texts), grounding

    # ------------------------------------------------------------ region head
    # Device-resident and batched: the heads are decode-regime GEMMs over B rows, "argmax the bin,
    # turn it into a value, Fourier-encode it" is one kernel (md_region_pick_encode), the decoder step
    # is md_text_forward -- no host round trip per coordinate (the reference syncs 3-4 times per
    # object: moondream.py:669,718-721).  One D2H per object decides whether every sequence is done.
    def _region(self):
        if self.w.region is None:
            raise NotImplementedError("checkpoint has no region head")
        if self._region_tables is None:
            r, rc = self.w.region, self.config.region
            nb_c, nb_s = rc.coord_out_dim, rc.size_out_dim // 2
            # bin -> value exactly as the reference computes it (moondream.py:673-674: argmax / size(-1),
            # fp32; :699-701: 2^(bin/1023*10-10), fp32), then the dtype of the logits (bf16)
            coord = (torch.arange(nb_c) / nb_c).to(BF16)
            size = torch.pow(2.0, (torch.arange(nb_s).float() / 1023.0) * 10.0 - 10.0).to(BF16)
            need = 0
            for lin in (r["coord_dec_fc1"], r["coord_dec_fc2"], r["size_dec_fc1"], r["size_dec_fc2"], r["coord_encoder"], r["size_encoder"]):
                st = lin.struct()
                need = max(need, self.lib.md_gemm_workspace_bytes(C.byref(st), 64, 1))
            self._region_tables = {
                "coord": coord.to(self._device), "size": size.to(self._device),
                # decode-regime split-K scratch: tickets start zeroed, every launch leaves them zeroed
                "splitk": torch.zeros(max(need, 16), dtype=torch.uint8, device=self._device),
            }
        return self.w.region, self._region_tables

    def _lin(self, a: torch.Tensor, lin, epi: int = _lib.MD_EPI_BIAS) -> torch.Tensor:
        """rows [m, k] (bf16, contiguous) -> [m, n] through md_gemm_bf16."""
        m = a.shape[0]
        if a.shape[1] != lin.k_pad or not a.is_contiguous():
            ap = torch.zeros(m, lin.k_pad, dtype=BF16, device=self._device)
            ap[:, : lin.k] = a
            a = ap
        _, tabs = self._region()
        ws = tabs["splitk"]
        out = torch.empty(m, lin.n_pad, dtype=BF16, device=self._device)
        args = _lib.MdGemmArgs(a.data_ptr(), lin.k_pad, lin.struct(), out.data_ptr(), lin.n_pad, None, 0, 0, m, epi, 1, 0,
                               ws.data_ptr(), ws.numel(), self._tile_policy)
        _lib.check(self.lib.md_gemm_bf16(C.byref(args), self._stream()), "md_gemm_bf16")
        return out[:, : lin.n]

    def _gemm(self, a, lin, epi: int = _lib.MD_EPI_BIAS):
        return self._lin(a.to(self._device, BF16), lin, epi)

    def _mlp(self, x: torch.Tensor, fc1, fc2) -> torch.Tensor:
        return self._lin(self._lin(x, fc1, _lib.MD_EPI_GELU), fc2)

    def _fourier(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """reference: region.py:12-29.  x bf16 [n, in_dim], w bf16 [in_dim, half] -> [n, 2*half]."""
        x = x.to(self._device, BF16).contiguous()
        n, in_dim = x.shape
        half = w.shape[1]
        out = torch.empty(n, 2 * half, dtype=BF16, device=self._device)
        _lib.check(
            self.lib.md_fourier_features(x.data_ptr(), x.stride(0), n, in_dim, w.data_ptr(), half, out.data_ptr(), out.stride(0), self._stream()),
            "md_fourier_features",
        )
        return out

    def encode_coordinate(self, coord: torch.Tensor) -> torch.Tensor:
        """reference: region.py:32-43."""
        r, _ = self._region()
        return self._lin(self._fourier(coord.reshape(-1, 1), r["coord_features"]), r["coord_encoder"])

    def decode_coordinate(self, hidden: torch.Tensor) -> torch.Tensor:
        """reference: region.py:46-57."""
        r, _ = self._region()
        return self._mlp(hidden.reshape(-1, hidden.shape[-1]).to(self._device, BF16), r["coord_dec_fc1"], r["coord_dec_fc2"])

    def encode_size(self, size: torch.Tensor) -> torch.Tensor:
        """reference: region.py:60-71."""
        r, _ = self._region()
        return self._lin(self._fourier(size.reshape(-1, 2), r["size_features"]), r["size_encoder"])

    def decode_size(self, hidden: torch.Tensor) -> torch.Tensor:
        """reference: region.py:74-93.  [1, D] -> [2, bins]; [B, D] -> [B, 2, bins]."""
        r, _ = self._region()
        h = hidden.reshape(-1, hidden.shape[-1]).to(self._device, BF16)
        out = self._mlp(h, r["size_dec_fc1"], r["size_dec_fc2"])
        return out.reshape(2, -1) if h.shape[0] == 1 else out.reshape(h.shape[0], 2, -1)

    def encode_spatial_refs(self, spatial_refs: SpatialRefs):
        """reference: region.py:96-136."""
        coords, sizes = [], []
        for ref in spatial_refs:
            if len(ref) == 2:
                coords += [ref[0], ref[1]]
            else:
                coords += [(ref[0] + ref[2]) / 2, (ref[1] + ref[3]) / 2]
                sizes.append([ref[2] - ref[0], ref[3] - ref[1]])
        c = self.encode_coordinate(torch.tensor(coords, dtype=BF16).view(-1, 1))
        s = self.encode_size(torch.tensor(sizes, dtype=BF16)) if sizes else None
        return {"coords": c, "sizes": s}

    def _region_pick_encode(self, hidden: torch.Tensor, which: str, bins_out: torch.Tensor,
                            logprobs_out: Optional[torch.Tensor] = None, window: int = 0) -> torch.Tensor:
        """hidden [B, D] -> next embedding [B, D]: head MLP -> per-sequence argmax bin(s) (written to
        ``bins_out`` [B, 1|2], int32) -> value -> Fourier features -> encoder.  All on the device.
        reference: moondream.py:672-677 (x), :682-687 (y), :693-713 (size).
        ``logprobs_out`` (fp32, the shape of ``bins_out``): the scored kernel instead -- the same bins and features, and
        the log of the mass the head put within ``window`` bins of each pick (md_region_pick_encode_scored)."""
        r, tabs = self._region()
        b = hidden.shape[0]
        if which == "coord":
            logits = self._mlp(hidden, r["coord_dec_fc1"], r["coord_dec_fc2"])
            groups, table, fw, enc = 1, tabs["coord"], r["coord_features"], r["coord_encoder"]
        else:
            logits = self._mlp(hidden, r["size_dec_fc1"], r["size_dec_fc2"])
            groups, table, fw, enc = 2, tabs["size"], r["size_features"], r["size_encoder"]
        n_bins = logits.shape[1] // groups
        half = fw.shape[1]
        feats = torch.empty(b, 2 * half, dtype=BF16, device=self._device)
        assert bins_out.dtype == torch.int32 and bins_out.stride(-1) == 1
        if logprobs_out is not None:
            assert logprobs_out.dtype == torch.float32 and logprobs_out.stride(-1) == 1 and logprobs_out.shape == bins_out.shape
            _lib.check(
                self.lib.md_region_pick_encode_scored(
                    logits.data_ptr(), logits.stride(0), b, groups, n_bins, table.data_ptr(), fw.data_ptr(), half,
                    bins_out.data_ptr(), bins_out.stride(0), feats.data_ptr(), feats.stride(0), window,
                    logprobs_out.data_ptr(), logprobs_out.stride(0), self._stream(),
                ),
                "md_region_pick_encode_scored",
            )
            return self._lin(feats, enc)
        _lib.check(
            self.lib.md_region_pick_encode(
                logits.data_ptr(), logits.stride(0), b, groups, n_bins, table.data_ptr(), fw.data_ptr(), half,
                bins_out.data_ptr(), bins_out.stride(0), feats.data_ptr(), feats.stride(0), self._stream(),
            ),
            "md_region_pick_encode",
        )
        return self._lin(feats, enc)

    def _points_loop(self, hidden: torch.Tensor, first: torch.Tensor, pos: Sequence[int], rows: Union[int, _Rows],
                     include_size: bool, max_objects: int, run_all: bool = False, scores: Optional[Scores] = None,
                     window: int = 0) -> Tuple[List[List[dict]], Optional[List[Optional[float]]]]:
        """The loop of moondream.py:653-733 for B sequences in lockstep.  hidden [B, D] = last prompt
        position, first int32 [B] = the token after the prompt, pos[b] = next position, ``rows`` their routing.
        Returns (every row's objects, None), or with scores (.., every row's ``stop_logprob``).
        ``scores`` (a record over [>= max_objects + 1, B] whose row 0 the prompt pass filled for ``first``): every object
        dict gains ``"logprobs"`` and ``"score"``, and the second result is each row's ``stop_logprob``.  Row k + 1 of the
        record takes the decision ``toks[k + 1]`` (one md_token_logprobs launch after the pick: the log-probability of the
        PICKED token, so of eos in the row the decision ends), a plane laid out like ``bins`` takes what
        md_region_pick_encode_scored writes at ``window``, and both travel in the one host copy with ``bins`` and ``toks``.
        Without ``scores`` the launches are the ones of the loop without the feature."""
        b = hidden.shape[0]
        eos = self.config.tokenizer.eos_id
        n_bins = self.config.region.coord_out_dim
        steps_per_obj = 3 if include_size else 2
        if max(pos) + steps_per_obj * max_objects > self.config.text.max_context:
            max_objects = max(0, (self.config.text.max_context - max(pos)) // steps_per_obj)
        bins = torch.zeros(max(1, max_objects), b, 4, dtype=torch.int32, device=self._device)
        toks = torch.full((max_objects + 1, b), eos, dtype=torch.int32, device=self._device)
        toks[0] = first
        lps = torch.zeros(max(1, max_objects), b, 4, dtype=torch.float32, device=self._device) if scores is not None else None
        lp_at = lambda k, c0, c1: {"logprobs_out": lps[k, :, c0:c1], "window": window} if lps is not None else {}
        pos_host = [int(p) for p in pos]
        pos_dev = torch.tensor(pos_host, dtype=torch.int32, device=self._device)
        hidden = hidden.reshape(b, -1).contiguous()

        def step(emb):
            nonlocal pos_host, hidden
            h = self._text_forward(emb.reshape(b, 1, -1), pos_host, rows, pos_dev=pos_dev)
            pos_host = [p + 1 for p in pos_host]
            pos_dev.add_(1)
            hidden = h.reshape(b, -1)

        n_done = 0
        for k in range(max_objects):
            # one host decision per object: is any sequence still emitting objects?
            # (run_all: benchmarks with a fixed amount of work -- every sequence runs max_objects rounds; what a
            # sequence emits after its eos is still dropped below)
            if not run_all:
                alive = (toks[: k + 1] != eos).all(dim=0)
                if not bool(alive.any()):
                    break
            step(self._region_pick_encode(hidden, "coord", bins[k, :, 0:1], **lp_at(k, 0, 1)))       # x -> y's hidden state
            emb = self._region_pick_encode(hidden, "coord", bins[k, :, 1:2], **lp_at(k, 1, 2))      # y
            if include_size:
                step(emb)
                emb = self._region_pick_encode(hidden, "size", bins[k, :, 2:4], **lp_at(k, 2, 4))    # w, h
            step(emb)
            logits = self._lm_head(hidden.reshape(b, 1, -1))
            toks[k + 1] = self._pick(logits, 0.0, 0.0)  # next token: x again, or eos
            if scores is not None:
                self._token_logprobs(logits, toks[k + 1], -1, scores.logprob[k + 1], scores.rank[k + 1])
            n_done = k + 1
        if scores is not None:  # bins, toks and both log-probability planes: ONE copy to the host
            host = scores[: n_done + 1].to_host(bins[:n_done], toks[: n_done + 1], lps[:n_done].view(torch.int32))
            bins_h, toks_h = (torch.from_numpy(a) for a in host.extra[:2])
            lps_h, tok_lp = host.extra[2].view(np.float32).astype(np.float64), host.logprob.astype(np.float64)
        else:
            bins_h = bins[:n_done].cpu() if n_done else torch.zeros(0, b, 4, dtype=torch.int32)
            toks_h = toks[: n_done + 1].cpu()
        # host floats exactly as the reference forms them (moondream.py:673,683,699-721)
        xc = (bins_h[..., 0].to(torch.int64) / n_bins)
        yc = (bins_h[..., 1].to(torch.int64) / n_bins)
        wv = torch.pow(2.0, (bins_h[..., 2].float() / 1023.0) * 10.0 - 10.0)
        hv = torch.pow(2.0, (bins_h[..., 3].float() / 1023.0) * 10.0 - 10.0)
        out: List[List[dict]] = []
        stops: Optional[List[Optional[float]]] = [] if scores is not None else None
        names = ("object", "x", "y", "w", "h") if include_size else ("object", "x", "y")
        for i in range(b):
            objs = []
            for k in range(n_done):
                if int(toks_h[k, i]) == eos:
                    break
                x, y = xc[k, i].item(), yc[k, i].item()
                if include_size:
                    w, h = wv[k, i].item(), hv[k, i].item()
                    objs.append({"x_min": x - w / 2, "y_min": y - h / 2, "x_max": x + w / 2, "y_max": y + h / 2})
                else:
                    objs.append({"x": x, "y": y})
                if scores is not None:
                    lp = dict(zip(names, [float(tok_lp[k, i])] + lps_h[k, i, : len(names) - 1].tolist()))
                    objs[-1].update(logprobs=lp, score=math.exp(math.fsum(lp.values())))
            if scores is not None:
                # the decision after the last object: eos ends the list, or max_objects / the context did (then no decision does)
                n = len(objs)  # <= n_done: toks_h has the row
                stops.append(float(tok_lp[n, i]) if int(toks_h[n, i]) == eos else None)
            out.append(objs)
        return out, stops

    # ------------------------------------------------- reasoning queries in lockstep
    def _region_coord(self) -> _lib.MdRegionCoord:
        """The coordinate half of the region head as md_decode_step_reason takes it (kept: a captured chunk bakes it in)."""
        if getattr(self, "_region_coord_struct", None) is None:
            r, tabs = self._region()
            fw = r["coord_features"]
            self._region_coord_struct = _lib.MdRegionCoord(
                r["coord_dec_fc1"].struct(), r["coord_dec_fc2"].struct(), r["coord_encoder"].struct(), fw.data_ptr(),
                tabs["coord"].data_ptr(), int(fw.shape[1]), int(self.config.region.coord_out_dim))
        return self._region_coord_struct

    def _reason_buffers(self, stream, b: int, n: int):
        """The fixed buffers of the reasoning loop: the rows' state per (stream, b) -- it lives across the chunks of a call
        -- and the per-step planes per (stream, b, n).  Captured chunks keep these addresses."""
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=self._device)
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self._device)
        state = self._store.fixed("reason", (stream, b), lambda: dict(
            phase=i32(b), n_reason=i32(b), n_answer=i32(b), suppress=i32(b, 2), coord_bin=i32(b), pos=i32(b),
            hidden_prev=torch.zeros(b, self.config.text.dim, dtype=BF16, device=self._device), temperature=f32(b), top_p=f32(b)))
        planes = self._store.fixed("reason", (stream, b, n), lambda: dict(
            tokens=i32(n + 1, b), kind=i32(n, b), ground=i32(n, b), forced=i32(n, b), uniforms=f32(n, b)))
        return state, planes

    def _reason_loop(self, hidden: torch.Tensor, first: torch.Tensor, pos: Sequence[int], rows: Union[int, _Rows], max_tokens: int,
                     sampling: Optional[Sampling] = None, forced: Optional[torch.Tensor] = None, check_every: int = 16,
                     on_chunk=None) -> List[dict]:
        """The loops of moondream.py:323-432 (reasoning), the suffix pass of :604 and :434-539 (answer) for B sequences as
        ONE lockstep decode loop with a phase per row (md_decode_step_reason), the counterpart of ``_points_loop``.
        ``hidden`` [B, D]: the last prompt position, ``first`` int32 [B]: the token picked from the prompt pass (nothing
        suppressed), ``pos[b]``: the next position, ``rows``: the routing.  ``max_tokens`` bounds each phase separately.
        At most 2 * max_tokens + 1 steps (every reasoning token, the suffix, every answer token), bounded by the context as
        ``_decode_greedy_impl`` bounds it, in chunks of ``check_every``: eager, or with ``compile()`` replayed from a captured
        graph; both over the fixed buffers of ``_reason_buffers``.  One D2H copy of the phases per chunk boundary decides
        whether every row is done.  ``sampling``: the call's settings (None: greedy); a sampled row draws one uniform per
        step, taken up front from the generator -- the step that feeds the suffix token consumes one like any other.
        ``forced``: int32 [steps, B], -1 = not forced: the token a step consumes instead of the picked one (tests).
        ``on_chunk(step0, n, state, planes)``: called after every chunk (tests: the buffers of the steps just run).
        Returns per row ``{"reasoning_ids", "answer_ids", "text", "grounding", "pos"}``: ``text`` / ``grounding`` as
        ``_generate_reasoning`` builds them, ``pos`` the position after the reasoning tokens (what it returns)."""
        rows = _Rows.of(rows)
        b = first.shape[0]
        t, tk = self.config.text, self.config.tokenizer
        self._ensure_batch(rows.span(b))
        pos_list = [int(p) for p in pos]
        assert len(pos_list) == b and hidden.shape[0] == b
        max_steps = max(0, min(2 * max_tokens + 1, t.max_context - 1 - max(pos_list)))
        region = self._region_coord()
        need = self.lib.md_decode_reason_workspace_bytes(C.byref(self.w.text), C.byref(region), b)
        graphs = self.use_graphs
        stream = torch.cuda.current_stream(self._device).cuda_stream
        per = max(1, min(check_every or 16, max(1, max_steps)))
        state, _ = self._reason_buffers(stream, b, per)
        state["phase"].fill_(_lib.MD_REASON_PHASE_REASON)
        state["n_reason"].zero_()
        state["n_answer"].zero_()
        state["suppress"].fill_(-1)
        state["hidden_prev"].copy_(hidden.reshape(b, -1))
        state["pos"].copy_(self._h2d(torch.tensor(pos_list, dtype=torch.int32)))
        state["temperature"].fill_(float(sampling.temperature) if sampling is not None else 0.0)
        state["top_p"].fill_(float(sampling.top_p) if sampling is not None else 1.0)
        pick = Sampling(state["temperature"], state["top_p"])
        uniforms = None
        if sampling is not None and max_steps:
            uniforms = torch.rand(max_steps, b, device=self._device, dtype=torch.float32, generator=sampling.generator)
            if sampling.row_perm is not None:
                uniforms = uniforms[:, sampling.row_perm].contiguous()
        if forced is not None:
            forced = forced.to(device=self._device, dtype=torch.int32)
            assert forced.dim() == 2 and forced.shape[1] == b
            if forced.shape[0] < max_steps:
                forced = torch.cat([forced, torch.full((max_steps - forced.shape[0], b), -1, dtype=torch.int32, device=self._device)])
        hist = torch.zeros(3, max_steps + 1, b, dtype=torch.int32, device=self._device)  # tokens, kind, ground (row i: step i)
        hist[0, 0] = first
        steps = 0
        while steps < max_steps:
            n = min(per, max_steps - steps)
            state, planes = self._reason_buffers(stream, b, n)
            planes["tokens"][0] = hist[0, steps]
            if uniforms is not None:
                planes["uniforms"].copy_(uniforms[steps : steps + n])
            if forced is not None:
                planes["forced"].copy_(forced[steps : steps + n])
            reason = ReasonChunk(state["phase"], state["n_reason"], state["n_answer"], state["suppress"], state["coord_bin"],
                                 state["hidden_prev"], planes["kind"], planes["ground"], max_tokens, max_tokens, region,
                                 planes["forced"] if forced is not None else None)
            chunk = DecodeChunk(b, planes["tokens"], state["pos"], lambda i: rows, -1, need, pick, planes["uniforms"], reason=reason)
            run_chunk(self, chunk, n, tag="reason", capture_stream=stream if graphs else None)
            hist[0, steps + 1 : steps + n + 1] = planes["tokens"][1:]
            hist[1, steps : steps + n] = planes["kind"]
            hist[2, steps : steps + n] = planes["ground"]
            if on_chunk is not None:
                on_chunk(steps, n, state, planes)
            steps += n
            if steps < max_steps and bool((state["phase"] == _lib.MD_REASON_PHASE_DONE).all()):
                break
        self.last_reason_steps = steps  # (tools/bench_reasoning.py: the decode steps the call ran)
        toks_h, kind_h, ground_h = hist[:, :steps].cpu().tolist() if steps else ([], [], [])
        forced_h = forced[:steps].cpu().tolist() if forced is not None and steps else None
        n_bins = self.config.region.coord_out_dim
        out = []
        for r in range(b):
            reasoning, answer = [], []
            text_chunks: List[List[int]] = [[]]
            bins: List[List[int]] = [[]]
            for i in range(steps):
                tok = forced_h[i][r] if forced_h is not None and forced_h[i][r] >= 0 else toks_h[i][r]
                if kind_h[i][r] == _lib.MD_REASON_KIND_REASON:
                    reasoning.append(tok)
                    if tok in (tk.start_ground_points_id, tk.end_ground_id):
                        text_chunks.append([])
                        bins.append([])
                    text_chunks[-1].append(tok)
                    if tok == tk.coord_id:
                        bins[-1].append(ground_h[i][r])
                elif kind_h[i][r] == _lib.MD_REASON_KIND_ANSWER:
                    answer.append(tok)
            texts = [self.tokenizer.decode(c) for c in text_chunks]
            grounding, start = [], 0
            for txt, bn in zip(texts, bins):
                g = (torch.tensor(bn, dtype=torch.int64) / n_bins).tolist()  # moondream.py:381: int64 / int, as a float
                if len(g) > 1:
                    pts = [(g[i], g[i + 1]) for i in range(0, len(g) - (len(g) % 2), 2)]
                    grounding.append({"start_idx": start, "end_idx": start + len(txt), "points": pts})
                start += len(txt)
            out.append({"reasoning_ids": reasoning, "answer_ids": answer, "text": "".join(texts), "grounding": grounding,
                        "pos": pos_list[r] + len(reasoning)})
        return out

    @staticmethod
    def _refuse_for_reasoning(settings: Optional[dict]) -> None:
        """What no reasoning query serves, the one-image ``query(reasoning=True)`` and the batched ones alike: ValueError."""
        refuse_settings(settings, {None: "reasoning queries", "filters": "reasoning queries (the reasoning loop picks with the "
                                   "call's temperature and top-p alone)"}, FAMILIES[:4] + ("stops",))

    def _check_reasoning_served(self, settings: Optional[dict]) -> None:
        """What the batched reasoning query does not serve raises NotImplementedError, naming the reason (ValueError for
        the penalty settings: a reasoning row's logits are masked per phase inside its own step)."""
        st = settings or {}
        self._refuse_for_reasoning(settings)
        if st.get("variant") is not None or st.get("variants") is not None:
            raise NotImplementedError("batched reasoning queries are not served with LoRA variants (variant / variants): "
                                      "use query(reasoning=True) per image")
        if self._kv8_scales is not None or bool(self.w.text.fp8) or bool(self.w.text.f8):
            raise NotImplementedError("batched reasoning queries are not served in the fp8 modes")
        tpl = self.config.tokenizer.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        if len(tpl["suffix"]) != 1:
            raise NotImplementedError(f"batched reasoning queries need a one-token query suffix (the suffix pass is one decode "
                                      f"step); this template's has {len(tpl['suffix'])} tokens")
        if self.w.region is None:
            raise NotImplementedError("batched reasoning queries need a region head (grounding): checkpoint has no region head")

    def _batch_query_reasoning(self, images, questions: Sequence[str], settings: Optional[dict], share_prefix: bool,
                               forced: Optional[torch.Tensor] = None, spatial_refs=None, built=None) -> List[dict]:
        """``batch_query(reasoning=True)`` / ``query_many_reasoning``: ``_reason_loop``'s rows in the caller's order.
        ``forced`` [steps, B] in the caller's row order (tests).  ``spatial_refs``: one entry per row, in front of the
        row's question as ``query(reasoning=True, spatial_refs=)`` places them; ``built``: their (prompts, record) when the
        caller has made them already (``_reasoning_prompts_spatial``)."""
        self._check_reasoning_served(settings)
        if len(images) != len(questions) or not len(images):
            raise ValueError("batch_query: one question per image, at least one")
        tk = self.config.tokenizer
        tpl = tk.templates["query"]
        spatial = built
        if spatial is None and spatial_refs is not None:
            spatial = self._reasoning_prompts_spatial(images, questions, spatial_refs)
        st = self._settings_of(settings, len(images))  # (what is left of them: everything else was refused above)
        # moondream.py:586-603: [prefix | question | suffix | thinking]
        prompts = [list(tpl["prefix"]) + list(self.tokenizer.encode(q).ids) + list(tpl["suffix"]) + [tk.thinking_id] for q in questions]
        if spatial is not None:
            prompts, spatial = spatial
        marks: list = []
        mark = lambda name: self._mark(marks, name)
        with torch.inference_mode():
            prep = self._prepare_sequences(images, prompts, mark, fuse=True, share_prefix=share_prefix, settings=st, spatial=spatial)
            if forced is not None:
                forced = forced.to(self._device)[:, torch.tensor(prep.order, device=self._device)]
            res = self._reason_loop(prep.hidden_last, prep.first, prep.next_pos, prep.rows, st.max_tokens, prep.sampling, forced)
            mark("reason_loop")
        self._phase_times(marks)
        return prep.in_caller_order(res)

    def _reasoning_prompts_spatial(self, images, questions: Sequence[str], spatial_refs):
        """``_query_prompts_spatial`` with the reasoning query's tail, [suffix | thinking] (moondream.py:593-603)."""
        tk = self.config.tokenizer
        tpl = tk.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        return self._query_prompts_spatial(images, questions, spatial_refs, list(tpl["suffix"]) + [tk.thinking_id])

    def _reasoning_answers(self, rows: List[dict]) -> List[dict]:
        """``_reason_loop``'s rows in the shape ``query(reasoning=True)`` returns."""
        return [{"reasoning": {"text": r["text"], "grounding": r["grounding"]}, "answer": self.tokenizer.decode(r["answer_ids"])}
                for r in rows]

    def _generate_points(self, hidden: torch.Tensor, next_token: torch.Tensor, pos: int, include_size: bool = True,
                         max_objects: int = DEFAULT_MAX_OBJECTS):
        """reference: moondream.py:653-733 (B = 1 form of the lockstep loop; KV slot 0)."""
        with torch.inference_mode():
            first = next_token.reshape(1).to(device=self._device, dtype=torch.int32)
            return self._points_loop(hidden.reshape(1, -1), first, [pos], 0, include_size, max_objects)[0][0]

    def _batch_detect_like(self, images, objects: Sequence[str], kind: str, include_size: bool, settings: Optional[dict],
                           share_prefix: bool = False) -> List[dict]:
        """``batch_detect`` / ``batch_point`` (and their one-image forms): the result dicts in the caller's order."""
        window = self._check_detect_settings(settings, kind)
        tpl = self.config.tokenizer.templates[kind]
        if tpl is None:
            raise NotImplementedError(f"Model does not support {kind}.")
        self._region()
        lora = self._lora(settings)  # moondream.py:757-761
        max_objects = (settings or {}).get("max_objects", DEFAULT_MAX_OBJECTS)
        prompts = [list(tpl["prefix"]) + list(self.tokenizer.encode(" " + o).ids) + list(tpl["suffix"]) for o in objects]
        marks: list = []
        mark = lambda name: self._mark(marks, name)
        with torch.inference_mode():
            scores = None
            if window is not None:  # row 0: the prompt pass's decision, row k + 1: the decision after object k
                n_rows = max(0, min(max_objects, self.config.text.max_context)) + 1
                scores = Scores.new((n_rows, len(prompts)), 0, self._device, fill=True)
            prep = self._prepare_sequences(images, prompts, mark, _Rows(lora=lora), share_prefix=share_prefix,
                                           encode_settings=settings, scores=scores and scores[0])
            res, stops = self._points_loop(prep.hidden_last, prep.first, prep.next_pos, prep.rows, include_size, max_objects,
                                           run_all=bool((settings or {}).get("_run_all_objects", False)), scores=scores,
                                           window=window or 0)
            mark("points_loop")
        self._phase_times(marks)
        key = "objects" if include_size else "points"
        if stops is None:
            return [{key: o} for o in prep.in_caller_order(res)]
        return [{key: o, "stop_logprob": s} for o, s in prep.in_caller_order(list(zip(res, stops)))]

    def _check_detect_settings(self, settings: Optional[dict], kind: str) -> Optional[int]:
        """The host checks of every detect / point call, before any GPU work: penalties are not served, and the score
        settings (``check_score_settings``) -> the score window, None without ``return_scores``."""
        refuse_settings(settings, {None: f"{kind}: its loop decodes coordinates, not tokens picked from logits",
                                   "filters": f"{kind}: its loop decodes coordinates, not tokens sampled from logits",
                                   "beams": f"{kind}: its loop decodes coordinates, not token hypotheses"}, FAMILIES[:4] + ("stops",))
        return check_score_settings(settings, self.config.region.coord_out_dim)

    def batch_detect(self, images, objects: Sequence[str], settings: Optional[dict] = None) -> List[dict]:
        """B (image, object) pairs in lockstep; element i == detect(images[i], objects[i]).

        ``settings={"return_scores": True}`` (here and in ``detect``, ``batch_point`` / ``point``, ``detect_many`` /
        ``point_many`` and ``batch_detect_pipelined``): every object dict gains ``"logprobs"`` -- ``"object"``, the
        log-probability of the token that opened the object (the prompt pass's pick for the first, the decision after the
        previous object for the others: the model's own distribution, md_token_logprobs), and ``"x"``, ``"y"`` (detect:
        ``"w"``, ``"h"`` too), the log of the mass the region head put within ``score_window`` bins (default 0: on exactly
        the picked bin) of each pick (md_region_pick_encode_scored) -- and ``"score"`` = exp(their sum), summed on the host in
        float64: at window 0 the probability the model gave to exactly this object given everything before it.  Every
        result dict gains ``"stop_logprob"``: log P(eos) at the decision that ended the list, None when ``max_objects`` or
        the context ended it.  Objects stay in emission order; no box or point changes, and without the setting the
        dicts, and the launches, are the ones of the call without the feature.  One launch more per object (the eos
        decision's md_token_logprobs), the scored pick in place of the plain one, the same single copy to the host.
        ValueError, before any GPU work: ``return_scores`` not a bool, ``score_window`` not an integer in
        0 .. coord_out_dim - 1, or given without ``return_scores``."""
        return self._batch_detect_like(images, objects, "detect", True, settings)

    def batch_point(self, images, objects: Sequence[str], settings: Optional[dict] = None) -> List[dict]:
        return self._batch_detect_like(images, objects, "point", False, settings)

    # ------------------------------------------------ one image, many prompts
    def query_many(self, image, questions: Sequence[str], settings: Optional[dict] = None) -> List[dict]:
        """Many questions about ONE image (reference pattern: encode_image once, then query per question,
        moondream.py:230-268,620-623), answered in one batch that reads a single copy of the image's KV prefix.  Element i ==
        ``{"answer": batch_query([encode_image(image)] * N, questions)[i]}``, in the bf16 mode and in the fp8 KV mode.  A LoRA
        ``variant`` (settings) takes the copy path, with the same results.  With reasoning: ``query_many_reasoning``.
        ``settings["spatial_refs"]``: one entry per question, ``batch_query``'s ``spatial_refs`` (the three-parameter
        signature is part of this call's contract) -- one image, N boxes and a question about each in one batch over one
        copy of the image's prefix."""
        spatial_refs = refs_of(settings)
        built = None
        if spatial_refs is not None:  # (built and checked, like everything below, before the image is encoded)
            built = self._query_prompts_spatial([image] * len(questions), questions, spatial_refs)
        prompts = built[0] if built is not None else self._query_prompts(questions)
        st = self._settings_of(settings, len(prompts))
        if built is not None and built[1] is not None and st.beams is not None:
            raise ValueError("num_beams > 1 (beam search) is not served with spatial_refs")
        enc = self.encode_image(image, settings)
        if built is not None:
            texts = self._string_ids_spatial([enc] * len(prompts), settings, built, st=st, share_prefix=True, text=True)
        else:
            texts = self._string_ids([enc] * len(prompts), prompts, settings, st, share_prefix=True, text=True)
        return [{"answer": t} for t in texts]

    def query_many_reasoning(self, image, questions: Sequence[str], settings: Optional[dict] = None, spatial_refs=None) -> List[dict]:
        """``query_many`` with reasoning: ``query(image, q, reasoning=True)`` for many questions about ONE image, in one
        lockstep batch over a single copy of the image's KV prefix.  Element i ==
        ``batch_query([encode_image(image)] * N, questions, settings, reasoning=True)[i]``; settings and refusals as there.
        (A method of its own: ``query_many``'s three-parameter signature is part of its contract.)  ``spatial_refs``: one
        entry per question, as ``batch_query`` takes them."""
        self._check_reasoning_served(settings)
        spatial_refs = refs_of(settings, spatial_refs)
        built = None
        if spatial_refs is not None:  # built and checked before the image is encoded
            built = self._reasoning_prompts_spatial([image] * len(questions), questions, spatial_refs)
        enc = self.encode_image(image, settings)
        return self._reasoning_answers(self._batch_query_reasoning([enc] * len(questions), questions, settings, share_prefix=True,
                                                                   built=built))

    def query_choices(self, image, question: str, choices: Sequence[str], settings: Optional[dict] = None, spatial_refs=None) -> dict:
        """Multiple choice: which of ``choices`` the model prefers as the answer to ``question`` about ONE image.  The image is
        encoded once; one row per choice over a single copy of its KV prefix (``score_ids`` with ``share_prefix``; a LoRA
        ``variant`` in ``settings`` takes the copy path, as in ``query_many``).  Every row's prompt is ``query``'s, its
        continuation the choice's tokens followed by ``eos_id`` -- a choice is scored as a COMPLETE answer.  No token is
        generated.  Returns ``{"logprobs": [sum per choice], "mean_logprobs": [sum / n_tokens], "per_token": [[..], ..],
        "best": argmax of logprobs, "best_normalized": argmax of mean_logprobs}`` (ties: the first choice).  The
        log-probabilities are ``score_ids``': the model's own distribution at temperature 1, untruncated.  ``spatial_refs``
        are not served here (ValueError)."""
        refuse_settings(settings, "score_ids / query_choices (the scorer's prompts carry no encoded references)", ("spatial_refs",),
                        spatial_refs=spatial_refs)
        choices = list(choices)
        if not choices:
            raise ValueError("query_choices: no choices")
        prompt = self._query_prompts([question])[0]
        eos = self.config.tokenizer.eos_id
        conts = [list(self.tokenizer.encode(c).ids) + [eos] for c in choices]
        enc = self.encode_image(image, settings)
        n = len(conts)
        per_token, _ = self.score_ids([enc] * n, [prompt] * n, conts, share_prefix=True, variant=(settings or {}).get("variant"))
        sums = [math.fsum(p) for p in per_token]
        means = [s_ / len(p) for s_, p in zip(sums, per_token)]
        return {"logprobs": sums, "mean_logprobs": means, "per_token": per_token,
                "best": max(range(n), key=lambda i: (sums[i], -i)), "best_normalized": max(range(n), key=lambda i: (means[i], -i))}

    def detect_many(self, image, objects: Sequence[str], settings: Optional[dict] = None) -> List[dict]:
        """``detect`` of many objects in ONE image over a single copy of its KV prefix.  Element i ==
        ``batch_detect([encode_image(image)] * N, objects)[i]`` (fp8 KV mode included).  LoRA variant: the copy path, same results."""
        self._check_detect_settings(settings, "detect")
        enc = self.encode_image(image, settings)
        return self._batch_detect_like([enc] * len(objects), objects, "detect", True, settings, True)

    def point_many(self, image, objects: Sequence[str], settings: Optional[dict] = None) -> List[dict]:
        """``point`` for many objects in ONE image over a single copy of its KV prefix.  Element i ==
        ``batch_point([encode_image(image)] * N, objects)[i]`` (fp8 KV mode included).  LoRA variant: the copy path, same results."""
        self._check_detect_settings(settings, "point")
        enc = self.encode_image(image, settings)
        return self._batch_detect_like([enc] * len(objects), objects, "point", False, settings, True)

    def batch_detect_pipelined(self, batches, settings: Optional[dict] = None, kind: str = "detect"):
        """Generator over an iterable of (images, objects) batches; yields ``batch_detect`` / ``batch_point`` (``kind``) of
        each, in order.  The detect counterpart of ``batch_generate_ids_pipelined``: while batch k runs on the GPU, the host
        tiling of batch k+1 (PIL LANCZOS resize + crop cutting of large images: ~19 ms of CPU per 768x1024 image, reference
        image_crops.py:124-167) is cut into pinned staging buffers by the background workers (``prefetch_crops``), so that
        only the first batch's tiling is exposed.  Results are identical to calling ``batch_detect`` per batch."""
        if kind not in ("detect", "point"):
            raise ValueError("kind must be 'detect' or 'point'")
        self._check_detect_settings(settings, kind)
        run = self.batch_detect if kind == "detect" else self.batch_point
        it = iter(batches)
        cur = next(it, None)
        try:
            while cur is not None:
                nxt = next(it, None)
                if nxt is not None:
                    nxt = (list(nxt[0]), list(nxt[1]))   # (the prefetch entry is keyed by these image objects' identities)
                    self.prefetch_crops(nxt[0])          # queued now, cut while the GPU runs ``cur``
                yield run(cur[0], cur[1], settings)
                cur = nxt
        finally:
            self.discard_prefetched_crops()              # a consumer that stops early: buffers returned

    def detect(self, image, object: str, settings: Optional[dict] = None):
        """reference: moondream.py:735-781."""
        return self.batch_detect([image], [object], settings)[0]

    def point(self, image, object: str, settings: Optional[dict] = None):
        """reference: moondream.py:783-829."""
        return self.batch_point([image], [object], settings)[0]
