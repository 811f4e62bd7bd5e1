"""VL support: the decoder-only text model of the oar-ocr-vl crate on HIP (lm_decode.hip) and, second stage, PaddleOCR-VL's vision
encoder and projector in front of it (vis_attention.hip, vis_host.cc).

`CausalLM` is PaddleOCR-VL's ERNIE-4.5 text decoder (oar-ocr-vl/src/models/paddleocr_vl/ernie.rs) and, by configuration, the Qwen2-VL
family's: RMSNorm, M-RoPE, grouped-query attention over a key / value cache, SwiGLU, greedy decoding.  `VisionEncoder` turns patches into
the decoder's input rows, `preprocess_images` RGB images into patches, `PaddleOCRVL.generate_tokens` images into generated token ids.
`QwenVisionEncoder`, `preprocess_images_qwen` and `QwenVL` are the same for the Qwen2-VL tower (MinerU2.5) and the windowed Qwen2.5-VL tower (NaviDC-OCR)
of oar-ocr-vl/src/backbones (qvis_misc.hip, qvis_host.cc).  The tokenizer and the chat template are not built: prompts are token ids."""
from __future__ import annotations

import ctypes as C
import json
import math
import struct
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import api

OAR_LM_F32, OAR_LM_BF16 = 1, 16
MAX_SEQUENCES = 16


class LmCfg(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("kv_heads", C.c_int32), ("head_dim", C.c_int32), ("intermediate", C.c_int32),
                ("vocab", C.c_int32), ("rms_eps", C.c_float), ("rope_theta", C.c_float), ("mrope_section", C.c_int32 * 3), ("qkv_bias", C.c_int32),
                ("tie_embeddings", C.c_int32), ("max_positions", C.c_int32), ("max_sequences", C.c_int32)]


class LmTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int32), ("rank", C.c_int32), ("dims", C.c_int64 * 4), ("data", C.c_void_p)]


class LmRequest(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("lengths", C.POINTER(C.c_int32)), ("inputs_embeds", C.POINTER(C.c_void_p)), ("input_ids", C.POINTER(C.c_void_p)),
                ("position_ids", C.POINTER(C.c_void_p)), ("max_new_tokens", C.c_int32), ("eos_token_id", C.c_int32), ("forced_tokens", C.c_void_p),
                ("logits", C.c_void_p), ("tokens", C.c_void_p), ("counts", C.c_void_p)]


class LmLogitsCfg(C.Structure):
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32), ("history_lengths", C.c_void_p), ("history_ids", C.POINTER(C.c_void_p))]


_bound = False
PREFILL_MODES = {"rows": 0, "gemm": 1}          # OAR_LM_PREFILL_ROWS / OAR_LM_PREFILL_GEMM
ATTENTION_MODES = {"serial": 0, "split": 1}     # OAR_LM_ATTN_SERIAL / OAR_LM_ATTN_SPLIT
SCHEDULES = ("groups", "refill")                # oar_lm_generate in groups of 16 / oar_lm_generate_queue
QUEUE_STATS = ("steps", "rows", "dead_rows", "admissions", "gemm_phases", "max_dead_rows", "min_slot_admissions", "min_slot_turnovers")   # oar_lm_queue_stats, in its order


def _lib():
    global _bound
    L = api.lib()
    if not _bound:
        L.oar_lm_create.restype = C.c_int
        L.oar_lm_create.argtypes = [C.POINTER(LmCfg), C.POINTER(LmTensor), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.oar_lm_destroy.restype = None
        L.oar_lm_destroy.argtypes = [C.c_void_p]
        L.oar_lm_generate.restype = C.c_int
        L.oar_lm_generate.argtypes = [C.c_void_p, C.POINTER(LmRequest)]
        L.oar_lm_cost.restype = C.c_int
        L.oar_lm_cost.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.oar_lm_set_prefill.restype = C.c_int
        L.oar_lm_set_prefill.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.oar_lm_prefill_cost.restype = C.c_int
        L.oar_lm_prefill_cost.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.oar_lm_set_decode.restype = C.c_int
        L.oar_lm_set_decode.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.oar_lm_decode_stats.restype = C.c_int
        L.oar_lm_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oar_lm_generate_queue.restype = C.c_int
        L.oar_lm_generate_queue.argtypes = [C.c_void_p, C.POINTER(LmRequest), C.c_int32]
        L.oar_lm_queue_check.restype = C.c_int
        L.oar_lm_queue_check.argtypes = [C.POINTER(LmCfg), C.POINTER(LmRequest), C.c_int32]
        if hasattr(L, "oar_lm_generate_ex"):   # (absent from a build of an earlier commit loaded through api.LIB_PATH)
            L.oar_lm_generate_ex.restype = C.c_int
            L.oar_lm_generate_ex.argtypes = [C.c_void_p, C.POINTER(LmRequest), C.POINTER(LmLogitsCfg)]
            L.oar_lm_logits_check.restype = C.c_int
            L.oar_lm_logits_check.argtypes = [C.POINTER(LmCfg), C.POINTER(LmRequest), C.POINTER(LmLogitsCfg)]
        L.oar_lm_queue_stats.restype = C.c_int
        L.oar_lm_queue_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
        _bound = True
    return L


GENERATION_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "eos_token_id")


def read_generation_defaults(path) -> dict:
    """What a `generation_config.json` in a checkpoint directory says about repetition_penalty, no_repeat_ngram_size and eos_token_id ({} without the file).
    Nothing applies these by itself: pass them to generate."""
    f = Path(path) / "generation_config.json"
    if not f.exists():
        return {}
    d = json.loads(f.read_text())
    return {k: d[k] for k in GENERATION_KEYS if d.get(k) is not None}


def _logits_cfg(n: int, repetition_penalty, no_repeat_ngram_size, history, keep) -> LmLogitsCfg:
    """The processors of a call over n sequences; history: None (the input ids), or one id sequence per sequence.  Arrays the struct points to go to `keep`."""
    lp = LmLogitsCfg()
    lp.repetition_penalty, lp.no_repeat_ngram_size = float(repetition_penalty), int(no_repeat_ngram_size)
    if history is not None:
        if len(history) != n:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"generate: {len(history)} histories for {n} sequences")
        hs = [np.ascontiguousarray(h, np.int32).reshape(-1) for h in history]
        lens = np.asarray([h.size for h in hs], np.int32)
        ptrs = (C.c_void_p * n)(*[h.ctypes.data if h.size else None for h in hs])
        keep += hs + [lens, ptrs]
        lp.history_lengths, lp.history_ids = lens.ctypes.data, C.cast(ptrs, C.POINTER(C.c_void_p))
    return lp


def _check_mode_names(prefill, decode_attention):
    """Unknown mode names are refused before anything else happens (no device needed)."""
    if isinstance(prefill, str) and prefill not in PREFILL_MODES:
        raise api.OCRError(api.OAR_INVALID_INPUT, f"prefill must be 'rows' or 'gemm', got {prefill!r}")
    if isinstance(decode_attention, str) and decode_attention not in ATTENTION_MODES:
        raise api.OCRError(api.OAR_INVALID_INPUT, f"decode_attention must be 'serial' or 'split', got {decode_attention!r}")


@dataclass
class CausalLMConfig:
    hidden_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    head_dim: int
    intermediate_size: int
    vocab_size: int
    rms_norm_eps: float = 1e-6
    rope_theta: float = 10000.0
    mrope_section: Sequence[int] = field(default_factory=list)   # empty: plain 1-D RoPE
    qkv_bias: bool = False
    tie_word_embeddings: bool = False
    max_positions: int = 4096
    max_sequences: int = MAX_SEQUENCES

    def __post_init__(self):
        if not list(self.mrope_section):
            self.mrope_section = [self.head_dim // 2, 0, 0]
        self.mrope_section = [int(v) for v in self.mrope_section]

    @classmethod
    def from_hf_json(cls, d: dict, **overrides) -> "CausalLMConfig":
        """A `config.json` in the shape of the reference's PaddleOcrVlConfig (oar-ocr-vl/src/models/paddleocr_vl/config.rs); `text_config`, where a
        checkpoint nests the text model's fields, is looked into first.  `use_bias` (ERNIE) / `attention_bias` become qkv_bias."""
        t = dict(d.get("text_config") or {})
        get = lambda k, default=None: t.get(k, d.get(k, default))   # noqa: E731
        heads = int(get("num_attention_heads"))
        hidden = int(get("hidden_size"))
        head_dim = int(get("head_dim") or hidden // heads)
        rs = get("rope_scaling") or {}
        sec = list(rs.get("mrope_section") or [])
        if sec and len(sec) != 3:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"rope_scaling.mrope_section must have 3 entries, got {sec}")
        kw = dict(hidden_size=hidden, num_hidden_layers=int(get("num_hidden_layers")), num_attention_heads=heads,
                  num_key_value_heads=int(get("num_key_value_heads") or heads), head_dim=head_dim, intermediate_size=int(get("intermediate_size")),
                  vocab_size=int(get("vocab_size")), rms_norm_eps=float(get("rms_norm_eps", 1e-6)), rope_theta=float(get("rope_theta", 10000.0)),
                  mrope_section=sec, qkv_bias=bool(get("use_bias", get("attention_bias", False))), tie_word_embeddings=bool(get("tie_word_embeddings", False)))
        kw.update(overrides)
        return cls(**kw)

    def to_c(self) -> LmCfg:
        c = LmCfg()
        c.hidden, c.layers, c.heads, c.kv_heads, c.head_dim = self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.num_key_value_heads, self.head_dim
        c.intermediate, c.vocab, c.rms_eps, c.rope_theta = self.intermediate_size, self.vocab_size, self.rms_norm_eps, self.rope_theta
        sec = list(self.mrope_section) + [0, 0, 0]
        for i in range(3):
            c.mrope_section[i] = int(sec[i])
        if len(self.mrope_section) != 3:
            c.mrope_section[0] = -1   # (refused by the library)
        c.qkv_bias, c.tie_embeddings, c.max_positions, c.max_sequences = int(self.qkv_bias), int(self.tie_word_embeddings), self.max_positions, self.max_sequences
        return c


# ---------------------------------------------------------------------------------- safetensors (8-byte length, JSON header, raw little-endian data)
_ST_DTYPES = {"F32": np.dtype("<f4"), "BF16": np.dtype("<u2"), "F16": np.dtype("<f2"), "F64": np.dtype("<f8"), "I64": np.dtype("<i8"), "I32": np.dtype("<i4"),
              "I16": np.dtype("<i2"), "I8": np.dtype("i1"), "U8": np.dtype("u1"), "BOOL": np.dtype("u1")}


def read_safetensors(path, names=None) -> Dict[str, np.ndarray]:
    """name -> array of one .safetensors file.  BF16 tensors come back as uint16 (their bit patterns); `names`: a predicate that selects tensors."""
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    if raw.size < 8:
        raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: too short for a safetensors file")
    (n,) = struct.unpack("<Q", bytes(raw[:8]))
    if n > raw.size - 8:
        raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: header length {n} exceeds the file")
    try:
        header = json.loads(bytes(raw[8:8 + n]).decode("utf-8"))
    except ValueError as e:
        raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: header is not JSON ({e})")
    out = {}
    data = raw[8 + n:]
    for name, info in header.items():
        if name == "__metadata__" or (names is not None and not names(name)):
            continue
        dt = _ST_DTYPES.get(info.get("dtype"))
        if dt is None:
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, f"{path}: tensor {name} has dtype {info.get('dtype')}")
        b, e = info["data_offsets"]
        shape = tuple(int(v) for v in info["shape"])
        count = int(np.prod(shape, dtype=np.int64))
        if not (0 <= b <= e <= data.size) or e - b != count * dt.itemsize:
            raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: tensor {name} has offsets {b}..{e} for shape {shape}")
        out[name] = np.frombuffer(data[b:e].tobytes(), dtype=dt).reshape(shape)
    return out


def _as_table_entry(name: str, t):
    """(array kept alive, dtype code): float32 stays, uint16 is bf16 bits, torch tensors are taken by value."""
    if hasattr(t, "detach"):   # a torch tensor
        import torch
        t = t.detach().cpu()
        if t.dtype == torch.bfloat16:
            return np.ascontiguousarray(t.contiguous().view(torch.int16).numpy().view(np.uint16)), OAR_LM_BF16
        return np.ascontiguousarray(t.to(torch.float32).numpy()), OAR_LM_F32
    a = np.asarray(t)
    if a.dtype == np.uint16:
        return np.ascontiguousarray(a), OAR_LM_BF16
    if a.dtype.kind == "f":
        return np.ascontiguousarray(a, np.float32), OAR_LM_F32
    raise api.OCRError(api.OAR_INVALID_INPUT, f"tensor {name}: dtype {a.dtype} is neither a float type nor uint16 (bf16 bits)")


def _tensor_table(tensors: dict, take, rename=None, reshape=None):
    """The LmTensor array of the tensors whose checkpoint name take(name) accepts -> (array, its length, the arrays it points into, to be kept alive until the
    library has copied them).  rename(name): the name the library looks up; reshape(name, array): the array as the library expects it, under that name (it may
    refuse the tensor by raising).  A tensor of a rank above 4 has no place in the struct and is left out."""
    keep, table = [], []
    for name, t in tensors.items():
        if not take(name):
            continue
        a, code = _as_table_entry(name, t)
        if rename is not None:
            name = rename(name)
        if reshape is not None:
            a = reshape(name, a)
        if a.ndim > 4:
            continue
        e = LmTensor()
        e.name, e.dtype, e.rank, e.data = name.encode(), code, a.ndim, a.ctypes.data
        for i, v in enumerate(a.shape):
            e.dims[i] = v
        keep.append(a)
        table.append(e)
    return (LmTensor * max(len(table), 1))(*table), len(table), keep


def _read_checkpoint(path, names=None) -> Dict[str, np.ndarray]:
    """Every *.safetensors file of a checkpoint directory as one name -> array dict; `names`: a predicate that selects tensors."""
    path = Path(path)
    files = sorted(path.glob("*.safetensors"))
    if not files:
        raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: no *.safetensors file")
    tensors = {}
    for f in files:
        tensors.update(read_safetensors(f, names=names))
    return tensors


class _Handle:
    """An owned handle of the library: destroy(handle) runs once, from close, the end of a `with` block or the collector."""

    def __init__(self, handle, destroy):
        self._h, self._destroy = handle, destroy

    def close(self):
        if self._h:
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@dataclass
class LMOutput:
    tokens: np.ndarray            # [n_seq, max_new_tokens] int32 (or [max_new_tokens] for a single sequence): eos from a sequence's first eos on
    counts: np.ndarray            # [n_seq] tokens up to and including the first eos
    logits: Optional[np.ndarray]  # [n_seq, max_new_tokens, vocab] float32 when asked for


class CausalLM(_Handle):
    def __init__(self, cfg: CausalLMConfig, handle):
        super().__init__(handle, lambda h: _lib().oar_lm_destroy(h))
        self.cfg = cfg
        self.generation_defaults: dict = {}   # from_dir: what the checkpoint's generation_config.json says (not applied by itself)

    @classmethod
    def from_state_dict(cls, cfg: CausalLMConfig, tensors: dict, prefix: str = "", device_id: int = 0) -> "CausalLM":
        """tensors: checkpoint name -> float array, uint16 array (bf16 bits) or torch tensor.  `prefix` is cut from the front of every name that has it
        (a checkpoint that nests the text model, e.g. "language_model.")."""
        if prefix:
            tensors = {name[len(prefix):]: t for name, t in tensors.items() if name.startswith(prefix)}
        arr, n, keep = _tensor_table(tensors, lambda name: name.startswith("model.") or name.startswith("lm_head."))
        h = C.c_void_p()
        api._check(_lib().oar_lm_create(C.byref(cfg.to_c()), arr, n, device_id, C.byref(h)))
        return cls(cfg, h)

    @classmethod
    def from_dir(cls, path, prefix: str = "", device_id: int = 0, **cfg_overrides) -> "CausalLM":
        """config.json + every *.safetensors of a checkpoint directory."""
        path = Path(path)
        cfg = CausalLMConfig.from_hf_json(json.loads((path / "config.json").read_text()), **cfg_overrides)
        tensors = _read_checkpoint(path, names=lambda n: n.startswith(prefix + "model.") or n.startswith(prefix + "lm_head."))
        lm = cls.from_state_dict(cfg, tensors, prefix=prefix, device_id=device_id)
        lm.generation_defaults = read_generation_defaults(path)
        return lm

    def cost(self, n_rows: int, cache_len: int):
        """(flops, bytes, launches) of one step of n_rows rows at cache_len cached positions."""
        f, b, n = C.c_double(), C.c_double(), C.c_int32()
        api._check(_lib().oar_lm_cost(self._h, n_rows, cache_len, C.byref(f), C.byref(b), C.byref(n)))
        return f.value, b.value, n.value

    def set_prefill(self, mode="rows", chunk_rows: Optional[int] = None):
        """How the following generate calls prefill: "rows" (the decode chain, 16 rows a step) or "gemm"  in chunks of chunk_rows packed
        rows (None: the default, 2048).  Integers reach the library as they are (it refuses what it does not know)."""
        code = PREFILL_MODES.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(code, str):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"prefill must be 'rows' or 'gemm', got {mode!r}")
        api._check(_lib().oar_lm_set_prefill(self._h, int(code), 0 if chunk_rows is None else int(chunk_rows)))

    def set_decode(self, attention="serial", split_keys: Optional[int] = None, stop_at_eos: bool = False):
        """How the following generate calls run their steps: attention "serial" (one launch, a workgroup walks a row's keys) or "split" (the keys cut
        into spans of split_keys, None: the default, 64; a second launch merges them); stop_at_eos: stop enqueuing steps once every sequence has emitted the
        call's eos_token_id.  Integers reach the library as they are (it refuses what it does not know)."""
        code = ATTENTION_MODES.get(attention, attention) if isinstance(attention, str) else attention
        if isinstance(code, str):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"decode_attention must be 'serial' or 'split', got {attention!r}")
        api._check(_lib().oar_lm_set_decode(self._h, int(code), 0 if split_keys is None else int(split_keys), int(stop_at_eos)))

    def decode_stats(self):
        """(steps_limit, steps_enqueued) of the last generate call: the steps it had scheduled and the steps it enqueued (fewer only when it stopped at eos)."""
        a, b = C.c_int64(), C.c_int64()
        api._check(_lib().oar_lm_decode_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def queue_stats(self):
        """Of the last generate call with schedule="refill" (DESIGN 4.44): steps and rows enqueued, dead rows (decode rows given to sequences after their eos
        step), admissions, GEMM phases, the most dead rows of one sequence, the fewest sequences one slot held and the
        fewest turnovers of one slot."""
        v = (C.c_int64 * len(QUEUE_STATS))()
        api._check(_lib().oar_lm_queue_stats(self._h, v, len(QUEUE_STATS)))
        return dict(zip(QUEUE_STATS, (int(x) for x in v)))

    def prefill_cost(self, lengths):
        """(flops, bytes, launches) of the GEMM phase of a call with these prompt lengths, at the chunk size set last."""
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        f, b, n = C.c_double(), C.c_double(), C.c_int32()
        api._check(_lib().oar_lm_prefill_cost(self._h, ln.size, ln.ctypes.data if ln.size else None, C.byref(f), C.byref(b), C.byref(n)))
        return f.value, b.value, n.value

    def generate(self, input_ids=None, inputs_embeds=None, position_ids=None, max_new_tokens: int = 16, eos_token_id: Optional[int] = None,
                 return_logits: bool = False, forced_tokens=None, logits_out: Optional[np.ndarray] = None, prefill: str = "rows",
                 prefill_chunk: Optional[int] = None, decode_attention: str = "serial", split_keys: Optional[int] = None, stop_at_eos: bool = False,
                 schedule: str = "groups", slots: Optional[int] = None, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, history_ids=None) -> LMOutput:
        """Greedy generation for one sequence or a list of sequences.  schedule "groups": more than 16 run in groups of 16, one after the other; "refill"
        (DESIGN 4.44): any number share `slots` cache slots (None: the model's max_sequences) and a finished sequence's slot goes to the next waiting one, with
        the same bytes per sequence, logits_out for any number of sequences, and stop_at_eos without meaning.  input_ids: [T] ints, or inputs_embeds: [T, hidden]
        floats; position_ids: [3, T] (default 0 .. T - 1 on all axes); forced_tokens: [max_new_tokens] per sequence, entries >= 0 are fed instead of the
        argmax.  logits_out: a flat float32 buffer of at least n_seq x max_new_tokens x vocab that receives the logits in place of a fresh array.
        prefill: "rows" or "gemm" with prefill_chunk packed rows a chunk (set_prefill); decode_attention: "serial" or "split" with split_keys keys a span, and
        stop_at_eos (set_decode); the model keeps the settings of its last call.
        repetition_penalty r >= 1 and no_repeat_ngram_size n (schedule "groups" only): before the arg-max every id of the sequence's history --
        history_ids (one id sequence per sequence; default: input_ids), then every token fed back -- has its logit x replaced by x < 0 ? x r : x / r, then the
        continuation of every earlier occurrence of the last n - 1 ids is banned.  Returned logits stay the raw logits.  The defaults are today's path."""
        _check_mode_names(prefill, decode_attention)
        if schedule not in SCHEDULES:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"schedule must be 'groups' or 'refill', got {schedule!r}")
        refill = schedule == "refill"
        processors = not (repetition_penalty == 1.0 and no_repeat_ngram_size == 0 and history_ids is None)
        if refill and (repetition_penalty != 1.0 or no_repeat_ngram_size > 1):
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, "generate: schedule 'refill' does not run the logits processors (a refilled slot's history is not re-seeded)")
        self.set_prefill(prefill, prefill_chunk)
        self.set_decode(decode_attention, split_keys, stop_at_eos)
        if (input_ids is None) == (inputs_embeds is None):
            raise api.OCRError(api.OAR_INVALID_INPUT, "generate: give exactly one of input_ids and inputs_embeds")
        src = input_ids if input_ids is not None else inputs_embeds
        single = not isinstance(src, (list, tuple)) or (input_ids is not None and len(src) > 0 and np.isscalar(src[0]))
        wrap = (lambda v: None if v is None else [v]) if single else (lambda v: v)
        seqs, pos, forced = wrap(src), wrap(position_ids), wrap(forced_tokens)
        hist = wrap(history_ids) if single and history_ids is not None and (len(history_ids) == 0 or np.isscalar(history_ids[0])) else history_ids
        n = len(seqs)
        if n == 0:
            raise api.OCRError(api.OAR_INVALID_INPUT, "generate: no sequence")
        if n > MAX_SEQUENCES and not refill:
            if logits_out is not None:
                raise api.OCRError(api.OAR_INVALID_INPUT, "generate: logits_out serves at most 16 sequences")
            outs = []
            for i in range(0, n, MAX_SEQUENCES):
                sl = slice(i, i + MAX_SEQUENCES)
                kw = {"input_ids" if input_ids is not None else "inputs_embeds": seqs[sl]}
                outs.append(self.generate(position_ids=None if pos is None else pos[sl], max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                                          return_logits=return_logits, forced_tokens=None if forced is None else forced[sl], prefill=prefill,
                                          prefill_chunk=prefill_chunk, decode_attention=decode_attention, split_keys=split_keys, stop_at_eos=stop_at_eos,
                                          repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                          history_ids=None if hist is None else list(hist[sl]), **kw))
            return LMOutput(np.concatenate([o.tokens for o in outs]), np.concatenate([o.counts for o in outs]),
                            np.concatenate([o.logits for o in outs]) if return_logits else None)
        V, D = self.cfg.vocab_size, self.cfg.hidden_size
        keep = []
        lengths = np.zeros(n, np.int32)
        ptrs = (C.c_void_p * n)()
        for i, s in enumerate(seqs):
            a = np.ascontiguousarray(s, np.int32) if input_ids is not None else np.ascontiguousarray(s, np.float32)
            if (input_ids is not None and a.ndim != 1) or (input_ids is None and (a.ndim != 2 or a.shape[1] != D)):
                raise api.OCRError(api.OAR_INVALID_INPUT, f"generate: sequence {i} has shape {a.shape}")
            keep.append(a)
            lengths[i] = a.shape[0]
            ptrs[i] = a.ctypes.data
        req = LmRequest()
        req.n_seq = n
        req.lengths = lengths.ctypes.data_as(C.POINTER(C.c_int32))
        if input_ids is not None:
            req.input_ids = C.cast(ptrs, C.POINTER(C.c_void_p))
        else:
            req.inputs_embeds = C.cast(ptrs, C.POINTER(C.c_void_p))
        if pos is not None:
            pp = (C.c_void_p * n)()
            for i, p in enumerate(pos):
                if p is None:
                    continue
                a = np.ascontiguousarray(p, np.int32)
                if a.shape != (3, int(lengths[i])):
                    raise api.OCRError(api.OAR_INVALID_INPUT, f"generate: position_ids of sequence {i} have shape {a.shape}, expected (3, {int(lengths[i])})")
                keep.append(a)
                pp[i] = a.ctypes.data
            keep.append(pp)
            req.position_ids = C.cast(pp, C.POINTER(C.c_void_p))
        req.max_new_tokens = int(max_new_tokens)
        req.eos_token_id = -1 if eos_token_id is None else int(eos_token_id)
        if forced is not None:
            f = np.full((n, max(int(max_new_tokens), 1)), -1, np.int32)
            for i, row in enumerate(forced):
                if row is not None:
                    r = np.asarray(row, np.int64)[:f.shape[1]]
                    f[i, :len(r)] = r
            keep.append(f)
            req.forced_tokens = f.ctypes.data
        tokens = np.zeros((n, max(int(max_new_tokens), 1)), np.int32)
        counts = np.zeros(n, np.int32)
        logits = None
        if return_logits or logits_out is not None:
            need = n * max(int(max_new_tokens), 1) * V
            if logits_out is not None:
                if logits_out.dtype != np.float32 or not logits_out.flags.c_contiguous or logits_out.size < need:
                    raise api.OCRError(api.OAR_INVALID_INPUT, "generate: logits_out must be contiguous float32 with room for the logits")
                logits = logits_out.reshape(-1)
            else:
                logits = np.empty(need, np.float32)
            req.logits = logits.ctypes.data
        req.tokens, req.counts = tokens.ctypes.data, counts.ctypes.data
        if refill:
            api._check(_lib().oar_lm_generate_queue(self._h, C.byref(req), 0 if slots is None else int(slots)))
        elif processors:
            api._check(_lib().oar_lm_generate_ex(self._h, C.byref(req), C.byref(_logits_cfg(n, repetition_penalty, no_repeat_ngram_size, hist, keep))))
        else:
            api._check(_lib().oar_lm_generate(self._h, C.byref(req)))
        if logits is not None:
            logits = logits[:n * tokens.shape[1] * V].reshape(n, tokens.shape[1], V)
        if single:
            return LMOutput(tokens[0], counts, None if logits is None else logits[0])
        return LMOutput(tokens, counts, logits)


# ================================================================================== the vision stage
MAX_IMAGES = 16
OAR_VIS_GELU_TANH, OAR_VIS_GELU_ERF = 0, 1


class VisCfg(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("intermediate", C.c_int32), ("patch", C.c_int32), ("channels", C.c_int32),
                ("pos_grid", C.c_int32), ("merge", C.c_int32), ("text_hidden", C.c_int32), ("ln_eps", C.c_float), ("act", C.c_int32), ("rope_theta", C.c_float),
                ("max_tokens", C.c_int32), ("max_images", C.c_int32)]


class VisRequest(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("grids", C.c_void_p), ("pixel_values", C.c_void_p), ("embeds", C.c_void_p), ("features", C.c_void_p)]


_vis_bound = False


def _vis_lib():
    global _vis_bound
    L = api.lib()
    if not _vis_bound:
        L.oar_vis_create.restype = C.c_int
        L.oar_vis_create.argtypes = [C.POINTER(VisCfg), C.POINTER(LmTensor), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.oar_vis_destroy.restype = None
        L.oar_vis_destroy.argtypes = [C.c_void_p]
        L.oar_vis_encode.restype = C.c_int
        L.oar_vis_encode.argtypes = [C.c_void_p, C.POINTER(VisRequest)]
        L.oar_vis_cost.restype = C.c_int
        L.oar_vis_cost.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        _vis_bound = True
    return L


@dataclass
class VisionConfig:
    hidden_size: int
    num_hidden_layers: int
    num_attention_heads: int
    intermediate_size: int
    patch_size: int
    text_hidden: int
    num_channels: int = 3
    pos_grid: int = 27                 # side of the learned position table (image_size // patch_size)
    spatial_merge_size: int = 2
    layer_norm_eps: float = 1e-6
    hidden_act: str = "gelu_pytorch_tanh"
    rope_theta: float = 10000.0
    max_tokens: int = 5120             # patches per call
    max_images: int = MAX_IMAGES

    @classmethod
    def from_hf_json(cls, d: dict, text_hidden: int, **overrides) -> "VisionConfig":
        """`config["vision_config"]` of a PaddleOCR-VL checkpoint (the reference's PaddleOcrVlVisionConfig)."""
        patch = int(d["patch_size"])
        kw = dict(hidden_size=int(d["hidden_size"]), num_hidden_layers=int(d["num_hidden_layers"]), num_attention_heads=int(d["num_attention_heads"]),
                  intermediate_size=int(d["intermediate_size"]), patch_size=patch, text_hidden=int(text_hidden), num_channels=int(d.get("num_channels", 3)),
                  pos_grid=int(d.get("image_size", 27 * patch)) // patch, spatial_merge_size=int(d.get("spatial_merge_size", 2)),
                  layer_norm_eps=float(d.get("layer_norm_eps", 1e-6)), hidden_act=str(d.get("hidden_act", "gelu_pytorch_tanh")))
        kw.update(overrides)
        return cls(**kw)

    def act_code(self) -> int:
        if self.hidden_act in ("gelu_pytorch_tanh", "gelu_new", "gelu_tanh"):
            return OAR_VIS_GELU_TANH
        if self.hidden_act == "gelu":
            return OAR_VIS_GELU_ERF
        raise api.OCRError(api.OAR_UNSUPPORTED_OP, f"vision hidden_act {self.hidden_act!r} is neither the tanh nor the erf GELU")

    def to_c(self) -> VisCfg:
        c = VisCfg()
        c.hidden, c.layers, c.heads, c.intermediate, c.patch, c.channels = self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size, self.patch_size, self.num_channels
        c.pos_grid, c.merge, c.text_hidden, c.ln_eps, c.act, c.rope_theta = self.pos_grid, self.spatial_merge_size, self.text_hidden, self.layer_norm_eps, self.act_code(), self.rope_theta
        c.max_tokens, c.max_images = self.max_tokens, self.max_images
        return c


@dataclass
class ImageProcessorConfig:
    patch_size: int = 14
    merge_size: int = 2
    min_pixels: int = 28 * 28 * 130
    max_pixels: int = 28 * 28 * 1280
    do_resize: bool = True
    do_rescale: bool = True
    do_normalize: bool = True
    rescale_factor: float = 1.0 / 255.0
    image_mean: Sequence[float] = (0.5, 0.5, 0.5)
    image_std: Sequence[float] = (0.5, 0.5, 0.5)
    resample: Optional[int] = None     # PIL's code; None: CatmullRom

    @classmethod
    def from_json(cls, d: dict) -> "ImageProcessorConfig":
        """a `preprocessor_config.json` (the reference's PaddleOcrVlImageProcessorConfig)"""
        names = ("patch_size", "merge_size", "min_pixels", "max_pixels", "do_resize", "do_rescale", "do_normalize", "rescale_factor", "image_mean", "image_std", "resample")
        cfg = cls(**{k: d[k] for k in names if k in d and d[k] is not None})
        if len(cfg.image_mean) != 3 or len(cfg.image_std) != 3 or any(float(v) == 0.0 for v in cfg.image_std):
            raise api.OCRError(api.OAR_INVALID_INPUT, "image_mean / image_std must have 3 entries and no zero std")
        if cfg.patch_size <= 0 or cfg.merge_size <= 0:
            raise api.OCRError(api.OAR_INVALID_INPUT, "patch_size and merge_size must be positive")
        return cfg


_PIL_RESAMPLE = {1: "lanczos3", 2: "triangle", 3: "catmullrom", 4: "triangle", 5: "catmullrom"}   # (box and hamming: the reference's stand-ins)


def smart_resize(height: int, width: int, factor: int, min_pixels: int, max_pixels: int):
    """-> (h, w), multiples of `factor` with min_pixels <= h w <= max_pixels where possible, in the reference's f64 arithmetic: round both sides to the factor
    (half away from zero); above max_pixels divide by beta = sqrt(h w / max_pixels) and floor, below min_pixels multiply by beta = sqrt(min_pixels / (h w)) and
    ceil; never below one factor."""
    if factor <= 0:
        raise api.OCRError(api.OAR_INVALID_INPUT, "smart_resize: factor must be > 0")
    h, w, f = float(height), float(width), float(factor)
    lo, hi = min(h, w), max(h, w)
    if lo > 0.0 and hi / lo > 200.0:
        raise api.OCRError(api.OAR_INVALID_INPUT, f"smart_resize: absolute aspect ratio must be <= 200, got {hi / lo:.3f}")
    rnd = lambda v: math.floor(v + 0.5)   # noqa: E731  (v >= 0)
    hb, wb = rnd(h / f) * f, rnd(w / f) * f
    if hb * wb > float(max_pixels):
        beta = math.sqrt((h * w) / float(max_pixels))
        hb, wb = max(math.floor((h / beta) / f) * f, f), max(math.floor((w / beta) / f) * f, f)
        if hb * wb < float(min_pixels):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"smart_resize: cannot satisfy both min_pixels={min_pixels} and max_pixels={max_pixels} constraints after quantization")
    elif hb * wb < float(min_pixels):
        beta = math.sqrt(float(min_pixels) / (h * w))
        hb, wb = max(math.ceil((h * beta) / f) * f, f), max(math.ceil((w * beta) / f) * f, f)
        if hb * wb > float(max_pixels):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"smart_resize: cannot satisfy both min_pixels={min_pixels} and max_pixels={max_pixels} constraints after quantization")
    return int(hb), int(wb)


def patchify(img_f32: np.ndarray, patch: int) -> np.ndarray:
    """[H, W, 3] -> [H/p W/p, 3 p p]: patch (gy, gx) in row-major order, its values in (c, dy, dx) order"""
    H, W, Cn = img_f32.shape
    gh, gw = H // patch, W // patch
    return np.ascontiguousarray(img_f32.reshape(gh, patch, gw, patch, Cn).transpose(0, 2, 4, 1, 3)).reshape(gh * gw, Cn * patch * patch)


def preprocess_images(images, cfg: ImageProcessorConfig, max_pixels: Optional[int] = None):
    """images: [H, W, 3] uint8 RGB arrays -> (pixel_values [sum h w, 3 p p] float32, grids [n, 2] int32 = (h, w) in patches).  Resize (smart_resize, through the
    library's exact resize kernel), then v * rescale_factor, then (v - mean) / std, each in f32 and in that order."""
    if len(images) == 0:
        raise api.OCRError(api.OAR_INVALID_INPUT, "preprocess_images: no images")
    p, factor = int(cfg.patch_size), int(cfg.patch_size) * int(cfg.merge_size)
    if cfg.resample is None:
        filt = "catmullrom"
    else:
        filt = _PIL_RESAMPLE.get(int(cfg.resample))
        if filt is None:
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, f"preprocess_images: resample code {cfg.resample} has no resize filter here")
    mean, std = np.asarray(cfg.image_mean, np.float32), np.asarray(cfg.image_std, np.float32)
    rows, grids = [], []
    for im in images:
        im = np.ascontiguousarray(im, np.uint8)
        if im.ndim != 3 or im.shape[2] != 3:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images: an image has shape {im.shape}, expected [H, W, 3]")
        h, w = im.shape[:2]
        rh, rw = smart_resize(h, w, factor, cfg.min_pixels, cfg.max_pixels if max_pixels is None else max_pixels) if cfg.do_resize else (h, w)
        if (rh, rw) != (h, w):
            im = api.k_resize_filter(im, rw, rh, filt)
        if rh % p or rw % p:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images: {rh}x{rw} is not divisible by patch_size={p}")
        v = im.astype(np.float32)
        if cfg.do_rescale:
            v = v * np.float32(cfg.rescale_factor)
        if cfg.do_normalize:
            v = (v - mean) / std
        rows.append(patchify(v, p))
        grids.append((rh // p, rw // p))
    return np.concatenate(rows), np.asarray(grids, np.int32).reshape(-1, 2)


def rope_index(input_ids, grids, image_token_id: int, vision_start_token_id: int, merge: int):
    """-> (positions [3, T] int32, delta): text runs count up on all three axes from the largest position so far + 1; the image tokens of a grid (h, w) get
    (base, base + hh, base + ww) over the merged grid (h / merge, w / merge); delta = largest position + 1 - T."""
    ids = [int(v) for v in np.asarray(input_ids).reshape(-1)]
    grids = [(int(h), int(w)) for h, w in np.asarray(grids, np.int64).reshape(-1, 2)]
    count = sum(1 for i in range(len(ids) - 1) if ids[i] == vision_start_token_id and ids[i + 1] == image_token_id)
    if count != len(grids):
        raise api.OCRError(api.OAR_INVALID_INPUT, f"rope_index: image count mismatch between prompt ({count}) and grids ({len(grids)})")
    pos, st, cur = [], 0, -1
    for n, (h, w) in enumerate(grids):
        try:
            ed = ids.index(image_token_id, st)
        except ValueError:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"rope_index: expected an image token for image {n} but none found")
        base0 = cur + 1
        for i in range(ed - st):
            pos.append((base0 + i,) * 3)
        cur = max(cur, base0 + ed - st - 1) if ed > st else cur
        base, lh, lw = base0 + ed - st, h // merge, w // merge
        for hh in range(lh):
            for ww in range(lw):
                pos.append((base, base + hh, base + ww))
        if lh * lw:
            cur = max(cur, base + max(lh, lw) - 1)
        st = ed + lh * lw
    base0 = cur + 1
    for i in range(st, len(ids)):
        pos.append((base0 + i - st,) * 3)
        cur = base0 + i - st
    if len(pos) != len(ids):
        raise api.OCRError(api.OAR_INVALID_INPUT, f"rope_index: position ids length mismatch: got {len(pos)}, expected {len(ids)}")
    return np.ascontiguousarray(np.asarray(pos, np.int32).reshape(-1, 3).T), cur + 1 - len(ids)


class _Encoder(_Handle):
    """cost and encode of a vision tower.  A subclass gives _fns() -> the library's (cost, encode) functions, _Request, its request struct, _widths() -> the
    floats of (a patch, an embedding row, a feature row), and _grids_ptr(g) -> what the library gets for the grids."""
    _Request = None

    def _grids_ptr(self, g):
        return g.ctypes.data

    def cost(self, grids):
        """(flops, bytes, launches) of one call over these grids."""
        g = np.ascontiguousarray(grids, np.int32).reshape(-1, 2)
        f, b, n = C.c_double(), C.c_double(), C.c_int32()
        api._check(self._fns()[0](self._h, g.shape[0], self._grids_ptr(g), C.byref(f), C.byref(b), C.byref(n)))
        return f.value, b.value, n.value

    def encode(self, pixel_values, grids, return_features: bool = False):
        """pixel_values [sum h w, patch width], grids [n, 2] -> embeds [sum h w / merge^2, output width] (and features [sum h w, tower width] when asked for);
        all images run in ONE call, packed back to back, and do not see each other.  The class says what order the rows are in."""
        g = np.ascontiguousarray(grids, np.int32).reshape(-1, 2)
        px = np.ascontiguousarray(pixel_values, np.float32)
        T = int((g[:, 0].astype(np.int64) * g[:, 1]).sum()) if g.size else 0
        kp, out_width, feat_width = self._widths()
        if px.size != T * kp:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"encode: pixel_values hold {px.size} floats, the grids need {T} x {kp}")
        m2 = self.cfg.spatial_merge_size ** 2
        emb = np.empty((max(T // m2, 0), out_width), np.float32)
        feat = np.empty((T, feat_width), np.float32) if return_features else None
        req = self._Request()
        req.n_images, req.grids, req.pixel_values, req.embeds = g.shape[0], self._grids_ptr(g), px.ctypes.data, emb.ctypes.data
        req.features = feat.ctypes.data if return_features else None
        api._check(self._fns()[1](self._h, C.byref(req)))
        return (emb, feat) if return_features else emb


class VisionEncoder(_Encoder):
    """PaddleOCR-VL's encoder and projector: pixel_values [sum h w, 3 p p] in raster order -> embeds [sum h w / merge^2, text_hidden], features [sum h w, hidden]."""
    _Request = VisRequest

    def __init__(self, cfg: VisionConfig, handle):
        super().__init__(handle, lambda h: _vis_lib().oar_vis_destroy(h))
        self.cfg = cfg

    def _fns(self):
        return _vis_lib().oar_vis_cost, _vis_lib().oar_vis_encode

    def _widths(self):
        return self.cfg.num_channels * self.cfg.patch_size ** 2, self.cfg.text_hidden, self.cfg.hidden_size

    @classmethod
    def from_state_dict(cls, cfg: VisionConfig, tensors: dict, device_id: int = 0) -> "VisionEncoder":
        """tensors: checkpoint name -> float array, uint16 array (bf16 bits) or torch tensor; the `visual.` and `mlp_AR.` names are taken."""
        arr, n, keep = _tensor_table(tensors, lambda name: name.startswith("visual.") or name.startswith("mlp_AR."))
        h = C.c_void_p()
        api._check(_vis_lib().oar_vis_create(C.byref(cfg.to_c()), arr, n, device_id, C.byref(h)))
        return cls(cfg, h)

    @classmethod
    def from_dir(cls, path, device_id: int = 0, **cfg_overrides) -> "VisionEncoder":
        path = Path(path)
        d = json.loads((path / "config.json").read_text())
        text_hidden = int((d.get("text_config") or {}).get("hidden_size", d.get("hidden_size")))
        cfg = VisionConfig.from_hf_json(d["vision_config"], text_hidden=text_hidden, **cfg_overrides)
        return cls.from_state_dict(cfg, _read_checkpoint(path, names=lambda n: n.startswith("visual.") or n.startswith("mlp_AR.")), device_id=device_id)


def _widen_rows(table: np.ndarray, ids) -> np.ndarray:
    rows = table[np.asarray(ids, np.int64)]
    if rows.dtype == np.uint16:   # bf16 bits
        return (rows.astype(np.uint32) << 16).view(np.float32)
    return np.ascontiguousarray(rows, np.float32)


def _generate_from_patches(model, px, grids, prefix_ids, suffix_ids, processors: bool, **gen) -> LMOutput:
    """What the composite models share behind their preprocessing (model: .vision with cfg.spatial_merge_size / max_images / max_tokens and encode, .lm,
    .embed_table, .image_token_id, .vision_start_token_id): the images are encoded in calls of at most max_images images and max_tokens patches; one sequence
    per image, ids = prefix + [image_token_id] x (h w / merge^2) + suffix, its embeddings the table rows with the image span replaced by the encoder's rows,
    its positions from rope_index; the expanded ids are the processors' history."""
    vis = model.vision
    m = vis.cfg.spatial_merge_size
    n_images = grids.shape[0]
    kp = px.shape[1]
    counts = grids[:, 0].astype(np.int64) * grids[:, 1]
    starts = np.concatenate([[0], np.cumsum(counts)])
    embeds = [None] * n_images
    i = 0
    while i < n_images:                                      # greedy groups: <= 16 images and <= max_tokens patches (a single larger image is refused by the library)
        j = i + 1
        while j < n_images and j - i < vis.cfg.max_images and starts[j + 1] - starts[i] <= vis.cfg.max_tokens:
            j += 1
        e = vis.encode(px[starts[i]:starts[j]].reshape(-1, kp), grids[i:j])
        off = 0
        for n in range(i, j):
            embeds[n] = e[off:off + counts[n] // (m * m)]
            off += counts[n] // (m * m)
        i = j
    seqs, pos, hist = [], [], []
    for n in range(n_images):
        n_img = int(counts[n]) // (m * m)
        ids = list(prefix_ids) + [model.image_token_id] * n_img + list(suffix_ids)
        x = _widen_rows(model.embed_table, ids)
        x[len(prefix_ids):len(prefix_ids) + n_img] = embeds[n]
        seqs.append(x)
        hist.append(np.asarray(ids, np.int32))
        pos.append(rope_index(ids, grids[n:n + 1], model.image_token_id, model.vision_start_token_id, m)[0])
    return model.lm.generate(inputs_embeds=seqs, position_ids=pos, history_ids=hist if processors else None, **gen)


class _ImagesToTokens:
    """A vision tower in front of a text decoder: images and token-id prompts in, generated token ids out.  A subclass gives from_state_dict and
    _preprocess(images) -> (pixel_values, grids)."""

    def __init__(self, vision, lm: CausalLM, embed_table: np.ndarray, preproc: ImageProcessorConfig, image_token_id: int, vision_start_token_id: int):
        self.vision, self.lm, self.embed_table, self.preproc = vision, lm, embed_table, preproc
        self.image_token_id, self.vision_start_token_id = int(image_token_id), int(vision_start_token_id)
        self.generation_defaults: dict = {}   # from_dir: the checkpoint's generation_config.json (not applied by itself)

    @classmethod
    def from_dir(cls, path, device_id: int = 0, **kw):
        path = Path(path)
        tensors = _read_checkpoint(path)
        m = cls.from_state_dict(json.loads((path / "config.json").read_text()), json.loads((path / "preprocessor_config.json").read_text()), tensors, device_id=device_id, **kw)
        m.generation_defaults = read_generation_defaults(path)
        m.lm.generation_defaults = dict(m.generation_defaults)
        return m

    def close(self):
        self.vision.close()
        self.lm.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def generate_tokens(self, images, prefix_ids, suffix_ids, max_new_tokens: int = 16, eos_token_id: Optional[int] = None, return_logits: bool = False, forced_tokens=None,
                        prefill: str = "rows", prefill_chunk: Optional[int] = None, decode_attention: str = "serial", split_keys: Optional[int] = None,
                        stop_at_eos: bool = False, schedule: str = "groups", slots: Optional[int] = None, repetition_penalty: float = 1.0,
                        no_repeat_ngram_size: int = 0) -> LMOutput:
        """One sequence per image: ids = prefix + [image_token_id] x (h w / merge^2) + suffix; its embeddings are the table rows with the image span replaced
        by the projector's rows, its positions come from rope_index.  The images are encoded in calls of at most 16 (and at most max_tokens patches).
        prefill / prefill_chunk / decode_attention / split_keys / stop_at_eos / schedule / slots: as CausalLM.generate; so are repetition_penalty and
        no_repeat_ngram_size, whose history is the expanded ids (prefix, one image id per image token, suffix)."""
        _check_mode_names(prefill, decode_attention)
        processors = repetition_penalty != 1.0 or no_repeat_ngram_size != 0
        if schedule == "refill" and (repetition_penalty != 1.0 or no_repeat_ngram_size > 1):
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, "generate_tokens: schedule 'refill' does not run the logits processors")
        px, grids = self._preprocess(images)
        return _generate_from_patches(self, px, grids, prefix_ids, suffix_ids, processors, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id, return_logits=return_logits,
                                      forced_tokens=forced_tokens, prefill=prefill, prefill_chunk=prefill_chunk, decode_attention=decode_attention, split_keys=split_keys,
                                      stop_at_eos=stop_at_eos, schedule=schedule, slots=slots, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)


class PaddleOCRVL(_ImagesToTokens):
    """Vision encoder + projector + text decoder: images and token-id prompts in, generated token ids out."""

    @classmethod
    def from_state_dict(cls, cfg_json: dict, preproc_json: dict, tensors: dict, device_id: int = 0, lm_overrides: Optional[dict] = None,
                        vision_overrides: Optional[dict] = None) -> "PaddleOCRVL":
        lm_cfg = CausalLMConfig.from_hf_json(cfg_json, **(lm_overrides or {}))
        vis_cfg = VisionConfig.from_hf_json(cfg_json["vision_config"], text_hidden=lm_cfg.hidden_size, **(vision_overrides or {}))
        table, _ = _as_table_entry("model.embed_tokens.weight", tensors["model.embed_tokens.weight"])
        vision = VisionEncoder.from_state_dict(vis_cfg, tensors, device_id=device_id)
        try:
            lm = CausalLM.from_state_dict(lm_cfg, tensors, device_id=device_id)
        except Exception:
            vision.close()
            raise
        return cls(vision, lm, table, ImageProcessorConfig.from_json(preproc_json), cfg_json["image_token_id"], cfg_json["vision_start_token_id"])

    def _preprocess(self, images):
        return preprocess_images(images, self.preproc)


# ================================================================================== the Qwen2-VL and Qwen2.5-VL vision towers
OAR_QVIS_QWEN2, OAR_QVIS_QWEN2_5 = 0, 1
QVIS_ACTS = {"quick_gelu": 0, "silu": 1, "gelu": 2, "gelu_new": 2, "gelu_pytorch_tanh": 2}   # (the reference implementation maps all three GELU names to the erf form)


class QvisCfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("embed", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("intermediate", C.c_int32), ("patch", C.c_int32),
                ("temporal_patch", C.c_int32), ("channels", C.c_int32), ("merge", C.c_int32), ("out_hidden", C.c_int32), ("act", C.c_int32), ("window_size", C.c_int32),
                ("n_fullatt", C.c_int32), ("fullatt_block_indexes", C.POINTER(C.c_int32)), ("rope_theta", C.c_float), ("max_tokens", C.c_int32), ("max_images", C.c_int32)]


class QvisRequest(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("grids", C.c_void_p), ("pixel_values", C.c_void_p), ("embeds", C.c_void_p), ("features", C.c_void_p)]


_qvis_bound = False


def _qvis_lib():
    global _qvis_bound
    L = api.lib()
    if not _qvis_bound:
        vp = C.c_void_p
        L.oar_qvis_create.restype = C.c_int
        L.oar_qvis_create.argtypes = [C.POINTER(QvisCfg), C.POINTER(LmTensor), C.c_int32, C.c_int32, C.POINTER(vp)]
        L.oar_qvis_destroy.restype = None
        L.oar_qvis_destroy.argtypes = [vp]
        L.oar_qvis_encode.restype = C.c_int
        L.oar_qvis_encode.argtypes = [vp, C.POINTER(QvisRequest)]
        L.oar_qvis_cost.restype = C.c_int
        L.oar_qvis_cost.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.oar_qvis_check.restype = C.c_int
        L.oar_qvis_check.argtypes = [C.POINTER(QvisCfg), C.c_int32, vp]
        L.oar_qvis_window_plan.restype = C.c_int
        L.oar_qvis_window_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        L.oar_k_qvis_rmsnorm.restype = C.c_int
        L.oar_k_qvis_rmsnorm.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_float, vp, C.c_size_t, C.c_size_t]
        L.oar_k_qvis_act.restype = C.c_int
        L.oar_k_qvis_act.argtypes = [vp, C.c_size_t, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_size_t, C.c_size_t]
        L.oar_k_qvis_row_gather.restype = C.c_int
        L.oar_k_qvis_row_gather.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int64, vp, C.c_size_t, C.c_size_t]
        _qvis_bound = True
    return L


@dataclass
class QwenVisionConfig:
    kind: str                          # "qwen2" (MinerU2.5) | "qwen2_5" (the windowed tower of NaviDC-OCR)
    embed_dim: int
    depth: int
    num_heads: int
    intermediate_size: int
    patch_size: int
    out_hidden_size: int               # the text model's hidden size
    temporal_patch_size: int = 2
    in_channels: int = 3
    spatial_merge_size: int = 2
    hidden_act: str = "quick_gelu"
    window_size: int = 0               # qwen2_5: pixels
    fullatt_block_indexes: Sequence[int] = field(default_factory=list)
    rope_theta: float = 10000.0
    max_tokens: int = 5120             # patches per call
    max_images: int = MAX_IMAGES

    @classmethod
    def from_hf_json(cls, d: dict, text_hidden: int, **overrides) -> "QwenVisionConfig":
        """`config["vision_config"]`.  The kind follows from the keys: window_size / out_hidden_size / intermediate_size mean qwen2_5 (hidden_size is then the
        tower's width, hidden_act defaults to silu); embed_dim / mlp_ratio mean qwen2 (intermediate = round(embed_dim mlp_ratio), hidden_size is the TEXT model's
        width, hidden_act defaults to quick_gelu).  in_chans or in_channels: the channel count."""
        chans = d.get("in_chans", d.get("in_channels", 3))
        common = dict(depth=int(d["depth"]), num_heads=int(d["num_heads"]), patch_size=int(d["patch_size"]), temporal_patch_size=int(d.get("temporal_patch_size", 2)),
                      in_channels=int(3 if chans is None else chans), spatial_merge_size=int(d.get("spatial_merge_size", 2)))
        if "window_size" in d or "out_hidden_size" in d or "intermediate_size" in d:
            kw = dict(kind="qwen2_5", embed_dim=int(d["hidden_size"]), intermediate_size=int(d["intermediate_size"]), out_hidden_size=int(d.get("out_hidden_size", text_hidden)),
                      hidden_act=str(d.get("hidden_act", "silu")), window_size=int(d["window_size"]), fullatt_block_indexes=[int(v) for v in d.get("fullatt_block_indexes", [])])
        elif "embed_dim" in d and "mlp_ratio" in d:
            kw = dict(kind="qwen2", embed_dim=int(d["embed_dim"]), intermediate_size=int(round(float(d["embed_dim"]) * float(d["mlp_ratio"]))),
                      out_hidden_size=int(d.get("hidden_size", text_hidden)), hidden_act=str(d.get("hidden_act", "quick_gelu")))
        else:
            raise api.OCRError(api.OAR_INVALID_INPUT, "vision_config has neither the Qwen2.5-VL keys (window_size, out_hidden_size, intermediate_size) nor the Qwen2-VL keys (embed_dim, mlp_ratio)")
        kw.update(common)
        kw.update(overrides)
        return cls(**kw)

    def act_code(self) -> int:
        code = QVIS_ACTS.get(self.hidden_act)
        if code is None:
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, f"unsupported vision hidden_act {self.hidden_act!r}")
        return code

    def to_c(self, keep: list, act: Optional[int] = None) -> QvisCfg:
        """keep: receives the array the struct points to"""
        if self.kind not in ("qwen2", "qwen2_5"):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"vision kind must be 'qwen2' or 'qwen2_5', got {self.kind!r}")
        c = QvisCfg()
        c.kind = OAR_QVIS_QWEN2_5 if self.kind == "qwen2_5" else OAR_QVIS_QWEN2
        c.embed, c.layers, c.heads, c.intermediate, c.patch, c.temporal_patch = self.embed_dim, self.depth, self.num_heads, self.intermediate_size, self.patch_size, self.temporal_patch_size
        c.channels, c.merge, c.out_hidden, c.act, c.window_size = self.in_channels, self.spatial_merge_size, self.out_hidden_size, self.act_code() if act is None else act, self.window_size
        full = np.ascontiguousarray(list(self.fullatt_block_indexes), np.int32)
        keep.append(full)
        c.n_fullatt = full.size
        c.fullatt_block_indexes = full.ctypes.data_as(C.POINTER(C.c_int32)) if full.size else None
        c.rope_theta, c.max_tokens, c.max_images = self.rope_theta, self.max_tokens, self.max_images
        return c

    @property
    def patch_dim(self) -> int:
        return self.in_channels * self.temporal_patch_size * self.patch_size ** 2


def qvis_check(cfg: QwenVisionConfig, grids=None, act: Optional[int] = None):
    """Every argument check of the library for this configuration (and these grids), without a device; raises OCRError.  act: a raw activation code."""
    keep = []
    g = None if grids is None else np.ascontiguousarray(grids, np.int32).reshape(-1, 2)
    ptr = None if g is None else (g if g.size else np.zeros(2, np.int32)).ctypes.data   # (grids given but empty: a request without images, which is refused)
    api._check(_qvis_lib().oar_qvis_check(C.byref(cfg.to_c(keep, act)), 0 if g is None else g.shape[0], ptr))


def qvis_window_plan(grids, merge: int, patch: int, window_size: int):
    """The library's window plan (host code, no device) -> (window_index, reverse_index, segments [(start, len)] in patches)."""
    g = np.ascontiguousarray(grids, np.int32).reshape(-1, 2)
    units = max(int((g[:, 0].astype(np.int64) // max(merge, 1) * (g[:, 1] // max(merge, 1))).sum()), 1) if g.size else 1
    wi, ri, ss, sl = (np.zeros(units, np.int32) for _ in range(4))
    n = C.c_int32()
    api._check(_qvis_lib().oar_qvis_window_plan(merge, patch, window_size, g.shape[0], g.ctypes.data if g.size else None, wi.ctypes.data, ri.ctypes.data, ss.ctypes.data, sl.ctypes.data, C.byref(n)))
    return wi, ri, [(int(a), int(b)) for a, b in zip(ss[:n.value], sl[:n.value])]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def k_qvis_rmsnorm(x, g, eps, o_io, o_off):
    """qvis_misc.hip: x [rows, d], g [d] -> o_io (a flat float32 array, written from o_off on); returns o_io"""
    x, g = _f32(x), _f32(g)
    api._check(_qvis_lib().oar_k_qvis_rmsnorm(x.ctypes.data, g.ctypes.data, x.shape[0], x.shape[1], eps, o_io.ctypes.data, o_io.size, o_off))
    return o_io


def k_qvis_act(buf, rows, f, act: str, gated: bool, o_io, o_off):
    """qvis_misc.hip: buf a flat float32 array that starts with [rows, f] (plain) or [rows, 2 f] (gated) -> o_io from o_off on; returns o_io"""
    buf = _f32(buf).reshape(-1)
    api._check(_qvis_lib().oar_k_qvis_act(buf.ctypes.data, buf.size, rows, f, QVIS_ACTS[act], int(gated), o_io.ctypes.data, o_io.size, o_off))
    return o_io


def k_qvis_row_gather(x, idx, o_io, o_off):
    """qvis_misc.hip: x [n_in, row_floats], idx [n] -> rows x[idx] in o_io from o_off on; returns o_io"""
    x, idx = _f32(x), np.ascontiguousarray(idx, np.int32).reshape(-1)
    api._check(_qvis_lib().oar_k_qvis_row_gather(x.ctypes.data, x.shape[0], x.shape[1], idx.ctypes.data, idx.size, o_io.ctypes.data, o_io.size, o_off))
    return o_io


class QwenVisionEncoder(_Encoder):
    """A Qwen2-VL or Qwen2.5-VL tower: pixel_values [sum h w, channels temporal p p] in merge-grouped order (preprocess_images_qwen) -> embeds
    [sum h w / merge^2, out_hidden] in raster order of the merged grids, features [sum h w, embed] (the last block's output in the caller's order)."""
    _Request = QvisRequest

    def __init__(self, cfg: QwenVisionConfig, handle):
        super().__init__(handle, lambda h: _qvis_lib().oar_qvis_destroy(h))
        self.cfg = cfg

    def _fns(self):
        return _qvis_lib().oar_qvis_cost, _qvis_lib().oar_qvis_encode

    def _widths(self):
        return self.cfg.patch_dim, self.cfg.out_hidden_size, self.cfg.embed_dim

    def _grids_ptr(self, g):   # (no grids: a null pointer, which the library refuses by name)
        return g.ctypes.data if g.size else None

    @classmethod
    def from_state_dict(cls, cfg: QwenVisionConfig, tensors: dict, prefix: str = "visual.", device_id: int = 0) -> "QwenVisionEncoder":
        """tensors: checkpoint name -> float array, uint16 array (bf16 bits) or torch tensor; the names under `prefix` are taken.  A 5-D patch weight
        [embed, channels, temporal, patch, patch] is taken as the [embed, channels temporal patch^2] matrix it is."""
        def reshape(name, a):
            if name == "patch_embed.proj.weight" and a.ndim > 2:
                a = a.reshape(a.shape[0], -1)
            if a.ndim > 4:
                raise api.OCRError(api.OAR_INVALID_INPUT, f"tensor {prefix}{name} has rank {a.ndim}: the tower has no tensor of a rank above 2 but the patch weight")
            return a
        arr, n, keep = _tensor_table(tensors, lambda name: name.startswith(prefix), rename=lambda name: name[len(prefix):], reshape=reshape)
        h = C.c_void_p()
        api._check(_qvis_lib().oar_qvis_create(C.byref(cfg.to_c(keep)), arr, n, device_id, C.byref(h)))
        return cls(cfg, h)

    @classmethod
    def from_dir(cls, path, prefix: str = "visual.", device_id: int = 0, **cfg_overrides) -> "QwenVisionEncoder":
        path = Path(path)
        d = json.loads((path / "config.json").read_text())
        text_hidden = int((d.get("text_config") or {}).get("hidden_size", d.get("hidden_size")))
        cfg = QwenVisionConfig.from_hf_json(d["vision_config"], text_hidden=text_hidden, **cfg_overrides)
        return cls.from_state_dict(cfg, _read_checkpoint(path, names=lambda n: n.startswith(prefix)), prefix=prefix, device_id=device_id)


def patchify_merge_grouped(img_f32: np.ndarray, patch: int, merge: int, temporal: int) -> np.ndarray:
    """[H, W, C] -> [H/p W/p, C temporal p p]: patches in (hb, wb, mi, mj) order, a patch's values in (c, tp, dy, dx) order with the one frame repeated"""
    H, W, Cn = img_f32.shape
    gh, gw = H // patch, W // patch
    v = img_f32.reshape(gh // merge, merge, patch, gw // merge, merge, patch, Cn).transpose(0, 3, 1, 4, 6, 2, 5)     # hb, wb, mi, mj, c, dy, dx
    v = np.repeat(v[:, :, :, :, :, None], temporal, 5)                                                               # ..., c, tp, dy, dx
    return np.ascontiguousarray(v).reshape(gh * gw, Cn * temporal * patch * patch)


def preprocess_images_qwen(images, cfg: ImageProcessorConfig, temporal_patch_size: int = 2, max_pixels: Optional[int] = None):
    """images: [H, W, 3] uint8 RGB arrays -> (pixel_values [sum h w, 3 temporal p p] float32 in merge-grouped order, grids [n, 2] int32 = (h, w) in patches): the
    resize path of preprocess_images (smart_resize with factor patch merge, the library's exact resize kernel), v * rescale_factor, (v - mean) / std, the frame
    repeated temporal_patch_size times.  With do_resize an image smaller than one factor is refused, as the reference implementation does."""
    if len(images) == 0:
        raise api.OCRError(api.OAR_INVALID_INPUT, "preprocess_images_qwen: no images")
    p, mg = int(cfg.patch_size), int(cfg.merge_size)
    factor = p * mg
    if temporal_patch_size < 1:
        raise api.OCRError(api.OAR_INVALID_INPUT, "preprocess_images_qwen: temporal_patch_size must be positive")
    if cfg.resample is None:
        filt = "catmullrom"
    else:
        filt = _PIL_RESAMPLE.get(int(cfg.resample))
        if filt is None:
            raise api.OCRError(api.OAR_UNSUPPORTED_OP, f"preprocess_images_qwen: resample code {cfg.resample} has no resize filter here")
    mean, std = np.asarray(cfg.image_mean, np.float32), np.asarray(cfg.image_std, np.float32)
    rows, grids = [], []
    for im in images:
        im = np.ascontiguousarray(im, np.uint8)
        if im.ndim != 3 or im.shape[2] != 3:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images_qwen: an image has shape {im.shape}, expected [H, W, 3]")
        h, w = im.shape[:2]
        if cfg.do_resize and (h < factor or w < factor):
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images_qwen: height/width must be >= factor {factor}, got {h}x{w}")
        rh, rw = smart_resize(h, w, factor, cfg.min_pixels, cfg.max_pixels if max_pixels is None else max_pixels) if cfg.do_resize else (h, w)
        if (rh, rw) != (h, w):
            im = api.k_resize_filter(im, rw, rh, filt)
        if rh % p or rw % p:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images_qwen: {rh}x{rw} is not divisible by patch_size={p}")
        if (rh // p) % mg or (rw // p) % mg:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"preprocess_images_qwen: the grid {rh // p}x{rw // p} is not divisible by merge_size={mg}")
        v = im.astype(np.float32)
        if cfg.do_rescale:
            v = v * np.float32(cfg.rescale_factor)
        if cfg.do_normalize:
            v = (v - mean) / std
        rows.append(patchify_merge_grouped(v, p, mg, int(temporal_patch_size)))
        grids.append((rh // p, rw // p))
    return np.concatenate(rows), np.asarray(grids, np.int32).reshape(-1, 2)


class QwenVL(_ImagesToTokens):
    """A Qwen2-VL (MinerU2.5) or Qwen2.5-VL (NaviDC-OCR) vision tower + the Qwen2 text decoder: images and token-id prompts in, generated token ids out.
    generation_defaults: what the checkpoint's generation_config.json says; nothing applies it.  (The reference implementation drives MinerU2.5 with
    no_repeat_ngram_size = 100 when generation_config.json is silent about it: pass it to generate_tokens to decode as it does.)"""

    @classmethod
    def from_state_dict(cls, cfg_json: dict, preproc_json: dict, tensors: dict, device_id: int = 0, lm_overrides: Optional[dict] = None,
                        vision_overrides: Optional[dict] = None, vision_prefix: str = "visual.") -> "QwenVL":
        """Qwen2 attention always has q / k / v biases and config.json does not say so (the reference implementation loads them unconditionally): qkv_bias is
        set here unless lm_overrides says otherwise."""
        lm_cfg = CausalLMConfig.from_hf_json(cfg_json, **{"qkv_bias": True, **(lm_overrides or {})})
        vis_cfg = QwenVisionConfig.from_hf_json(cfg_json["vision_config"], text_hidden=lm_cfg.hidden_size, **(vision_overrides or {}))
        table, _ = _as_table_entry("model.embed_tokens.weight", tensors["model.embed_tokens.weight"])
        pj = dict(preproc_json)
        size = pj.get("size") or {}
        if "shortest_edge" in size and "longest_edge" in size:   # (the newer spelling of min_pixels / max_pixels, which the reference implementation reads first)
            pj["min_pixels"], pj["max_pixels"] = int(size["shortest_edge"]), int(size["longest_edge"])
        preproc = ImageProcessorConfig.from_json(pj)
        if int(pj.get("temporal_patch_size", vis_cfg.temporal_patch_size)) != vis_cfg.temporal_patch_size:
            raise api.OCRError(api.OAR_INVALID_INPUT, "the preprocessor's temporal_patch_size differs from the vision tower's")
        vision = QwenVisionEncoder.from_state_dict(vis_cfg, tensors, prefix=vision_prefix, device_id=device_id)
        try:
            lm = CausalLM.from_state_dict(lm_cfg, tensors, device_id=device_id)
        except Exception:
            vision.close()
            raise
        return cls(vision, lm, table, preproc, cfg_json["image_token_id"], cfg_json["vision_start_token_id"])

    def _preprocess(self, images):
        return preprocess_images_qwen(images, self.preproc, self.vision.cfg.temporal_patch_size)
