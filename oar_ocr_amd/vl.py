"""VL support, first stage: the decoder-only text model of the oar-ocr-vl crate on HIP (lm_decode.hip).

`CausalLM` is PaddleOCR-VL's ERNIE-4.5 text decoder (oar-ocr-vl/src/models/paddleocr_vl/ernie.rs) and, by configuration, the Qwen2-VL
family's: RMSNorm, M-RoPE, grouped-query attention over a key / value cache, SwiGLU, greedy decoding.  The vision encoder, the projector,
image preprocessing, the tokenizer and the chat template are not built: `generate` takes token ids or ready `inputs_embeds`."""
from __future__ import annotations

import ctypes as C
import json
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


_bound = False


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
        _bound = True
    return L


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


@dataclass
class LMOutput:
    tokens: np.ndarray            # [n_seq, max_new_tokens] int32 (or [max_new_tokens] for a single sequence): eos from a sequence's first eos on
    counts: np.ndarray            # [n_seq] tokens up to and including the first eos
    logits: Optional[np.ndarray]  # [n_seq, max_new_tokens, vocab] float32 when asked for


class CausalLM:
    def __init__(self, cfg: CausalLMConfig, handle):
        self.cfg, self._h = cfg, handle

    @classmethod
    def from_state_dict(cls, cfg: CausalLMConfig, tensors: dict, prefix: str = "", device_id: int = 0) -> "CausalLM":
        """tensors: checkpoint name -> float array, uint16 array (bf16 bits) or torch tensor.  `prefix` is cut from the front of every name that has it
        (a checkpoint that nests the text model, e.g. "language_model.")."""
        keep, table = [], []
        for name, t in tensors.items():
            if prefix:
                if not name.startswith(prefix):
                    continue
                name = name[len(prefix):]
            if not (name.startswith("model.") or name.startswith("lm_head.")):
                continue
            a, code = _as_table_entry(name, t)
            if a.ndim > 4:
                continue
            e = LmTensor()
            e.name, e.dtype, e.rank, e.data = name.encode(), code, a.ndim, a.ctypes.data
            for i, v in enumerate(a.shape):
                e.dims[i] = v
            keep.append(a)
            table.append(e)
        arr = (LmTensor * max(len(table), 1))(*table)
        h = C.c_void_p()
        api._check(_lib().oar_lm_create(C.byref(cfg.to_c()), arr, len(table), device_id, C.byref(h)))
        return cls(cfg, h)

    @classmethod
    def from_dir(cls, path, prefix: str = "", device_id: int = 0, **cfg_overrides) -> "CausalLM":
        """config.json + every *.safetensors of a checkpoint directory."""
        path = Path(path)
        cfg = CausalLMConfig.from_hf_json(json.loads((path / "config.json").read_text()), **cfg_overrides)
        files = sorted(path.glob("*.safetensors"))
        if not files:
            raise api.OCRError(api.OAR_MODEL_LOAD, f"{path}: no *.safetensors file")
        want = lambda n: n.startswith(prefix + "model.") or n.startswith(prefix + "lm_head.")   # noqa: E731
        tensors = {}
        for f in files:
            tensors.update(read_safetensors(f, names=want))
        return cls.from_state_dict(cfg, tensors, prefix=prefix, device_id=device_id)

    def close(self):
        if self._h:
            _lib().oar_lm_destroy(self._h)
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

    def cost(self, n_rows: int, cache_len: int):
        """(flops, bytes, launches) of one step of n_rows rows at cache_len cached positions."""
        f, b, n = C.c_double(), C.c_double(), C.c_int32()
        api._check(_lib().oar_lm_cost(self._h, n_rows, cache_len, C.byref(f), C.byref(b), C.byref(n)))
        return f.value, b.value, n.value

    def generate(self, input_ids=None, inputs_embeds=None, position_ids=None, max_new_tokens: int = 16, eos_token_id: Optional[int] = None,
                 return_logits: bool = False, forced_tokens=None, logits_out: Optional[np.ndarray] = None) -> LMOutput:
        """Greedy generation for one sequence or a list of sequences (more than 16 run in groups of 16).  input_ids: [T] ints, or inputs_embeds: [T, hidden]
        floats; position_ids: [3, T] (default 0 .. T - 1 on all axes); forced_tokens: [max_new_tokens] per sequence, entries >= 0 are fed instead of the
        argmax.  logits_out: a flat float32 buffer of at least n_seq x max_new_tokens x vocab that receives the logits in place of a fresh array."""
        if (input_ids is None) == (inputs_embeds is None):
            raise api.OCRError(api.OAR_INVALID_INPUT, "generate: give exactly one of input_ids and inputs_embeds")
        src = input_ids if input_ids is not None else inputs_embeds
        single = not isinstance(src, (list, tuple)) or (input_ids is not None and len(src) > 0 and np.isscalar(src[0]))
        wrap = (lambda v: None if v is None else [v]) if single else (lambda v: v)
        seqs, pos, forced = wrap(src), wrap(position_ids), wrap(forced_tokens)
        n = len(seqs)
        if n == 0:
            raise api.OCRError(api.OAR_INVALID_INPUT, "generate: no sequence")
        if n > MAX_SEQUENCES:
            if logits_out is not None:
                raise api.OCRError(api.OAR_INVALID_INPUT, "generate: logits_out serves at most 16 sequences")
            outs = []
            for i in range(0, n, MAX_SEQUENCES):
                sl = slice(i, i + MAX_SEQUENCES)
                kw = {"input_ids" if input_ids is not None else "inputs_embeds": seqs[sl]}
                outs.append(self.generate(position_ids=None if pos is None else pos[sl], max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                                          return_logits=return_logits, forced_tokens=None if forced is None else forced[sl], **kw))
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
        api._check(_lib().oar_lm_generate(self._h, C.byref(req)))
        if logits is not None:
            logits = logits[:n * tokens.shape[1] * V].reshape(n, tokens.shape[1], V)
        if single:
            return LMOutput(tokens[0], counts, None if logits is None else logits[0])
        return LMOutput(tokens, counts, logits)
