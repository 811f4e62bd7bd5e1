"""Formula recognition: `FormulaRecognitionAdapter` (domain/adapters/formula_recognition_adapter.rs) over `PPFormulaNetModel`
(models/recognition/pp_formulanet.rs) with `FormulaPreprocessor` and `normalize_latex` (processors/formula_preprocess.rs), and over `UniMERNetModel`
(models/recognition/unimernet.rs) with `UniMERNetPreprocessor` (processors/unimernet_preprocess.rs): `FormulaRecognitionPredictor(model_type="unimernet")`.

A PP-FormulaNet file is one ONNX graph from image to token ids: the greedy decode sits inside it as a Loop, which the engine runs as its FormulaDecode
operator (csrc/formula_decode.hip).  Everything here is host orchestration around `api.OrtInfer`: margin crop, Triangle resize through the
existing `api.k_resize_triangle`, the f32 normalisation in the reference's operation order, the token filter, a ByteLevel tokenizer decode and the LaTeX
clean-up.  The host stops at eos.  The graph runs all its steps unless the predictor is built with `stop_at_eos=True`: the engine then ends a chunk of 16
images once each of them has emitted eos (`api.OrtInfer.set_decode_stop`) and fills the rest of their rows with eos, which the token filter never reads.

Not pinned against the reference's dependencies: `to_luma8` of a pixel that is not grey (the image crate's integer weights are restated here from its
documentation: (2126 R + 7152 G + 722 B) / 10000; a grey pixel maps to itself under any weights that sum to one), and the spelling of the real
`pp-formulanet*.onnx` and `unimernet.onnx` files, and what the image crate does when a resize target truncates to 0 pixels (here: an
all-white canvas for UniMERNet, an all-black one for PP-FormulaNet).  Tokenizers whose decoder is not ByteLevel are not built."""
from __future__ import annotations

import json
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import api

F = np.float32


@dataclass
class FormulaRecognitionConfig:
    """domain/tasks/formula_recognition.rs: score_threshold is carried but cannot be applied (the model yields no scores)."""
    score_threshold: float = 0.0
    max_length: int = 1536
    batch_size: int = 8


@dataclass
class FormulaRecognitionOutput:
    formulas: List[str] = field(default_factory=list)
    scores: List[Optional[float]] = field(default_factory=list)     # always None (formula_recognition_adapter.rs:256-260)


@dataclass
class FormulaResult:
    """domain/structure.rs:2616-2623"""
    bbox: np.ndarray
    latex: str
    confidence: float


# ------------------------------------------------------------------------------------------------ preprocessing
def _as_u8(v: np.ndarray) -> np.ndarray:
    """Rust `f32 as u8`: truncation toward zero, saturating, NaN -> 0."""
    v = np.nan_to_num(np.asarray(v, np.float32), nan=0.0)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def _as_u32(v) -> int:
    v = float(v)
    if v != v or v <= 0.0:
        return 0
    return min(int(v), 0xFFFFFFFF)


def to_luma8(rgb: np.ndarray) -> np.ndarray:
    """DynamicImage::to_luma8 of an RGB8 image (see the module docstring: unpinned for pixels that are not grey)."""
    c = np.asarray(rgb, np.uint8).astype(np.uint32)
    return ((2126 * c[..., 0] + 7152 * c[..., 1] + 722 * c[..., 2]) // 10000).astype(np.uint8)


class FormulaPreprocessor:
    """formula_preprocess.rs:50-256.  target_size is (width, height), as in the reference."""

    def __init__(self, target_size=(384, 384), crop_threshold: int = 200, padding_multiple: int = 16, normalize_mean=(0.7931, 0.7931, 0.7931),
                 normalize_std=(0.1738, 0.1738, 0.1738)):
        self.target_size = (int(target_size[0]), int(target_size[1]))
        self.crop_threshold = int(crop_threshold)
        self.padding_multiple = int(padding_multiple)
        self.mean = np.asarray(normalize_mean, np.float32)
        self.std = np.asarray(normalize_std, np.float32)

    def crop_rect(self, img: np.ndarray):
        """:78-135 -> (x, y, w, h) of the foreground box, or None where the reference returns the image as it is"""
        gray = to_luma8(img)
        if gray.size == 0:
            return None
        mn, mx = gray.min(), gray.max()
        if mx == mn:
            return None
        norm = _as_u8((gray.astype(np.float32) - F(mn)) / F(F(mx) - F(mn)) * F(255.0))
        ys, xs = np.nonzero(norm < self.crop_threshold)
        if ys.size == 0:
            return None
        x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
        if x0 >= x1 or y0 >= y1:
            return None
        return x0, y0, x1 - x0 + 1, y1 - y0 + 1

    def crop_margin(self, img: np.ndarray) -> np.ndarray:
        r = self.crop_rect(img)
        if r is None:
            return img
        x, y, w, h = r
        return np.ascontiguousarray(img[y:y + h, x:x + w])

    def resized_size(self, w: int, h: int):
        """:147-154 -> (final_width, final_height): f32 scale, truncating casts"""
        tw, th = self.target_size
        scale = F(F(min(tw, th)) / F(max(w, h)))
        return min(_as_u32(F(F(w) * scale)), tw), min(_as_u32(F(F(h) * scale)), th)

    def resize_and_pad(self, img: np.ndarray) -> np.ndarray:
        """:139-169 -> RGB [th, tw, 3], the resized image centred on black"""
        tw, th = self.target_size
        h, w = img.shape[:2]
        out = np.zeros((th, tw, 3), np.uint8)
        if w == 0 or h == 0:
            return out
        fw, fh = self.resized_size(w, h)
        if fw == 0 or fh == 0:
            return out
        left, top = (tw - fw) // 2, (th - fh) // 2
        # (a Triangle resize to the same size is the identity: its kernel is 1 at the sample itself and 0 at every neighbour)
        out[top:top + fh, left:left + fw] = img[..., :3] if (fw, fh) == (w, h) else api.k_resize_triangle(img, fw, fh)
        return out

    def normalize_and_to_grayscale(self, img: np.ndarray) -> np.ndarray:
        """:174-222 -> [h, w] f32 (the reference replicates it to three equal channels and keeps the first)"""
        c = np.asarray(img, np.uint8).astype(np.float32)
        scale = F(1.0) / F(255.0)
        std = np.maximum(self.std, np.finfo(np.float32).eps)
        b = (c[..., 2] * scale - self.mean[0]) / std[0]
        g = (c[..., 1] * scale - self.mean[1]) / std[1]
        r = (c[..., 0] * scale - self.mean[2]) / std[2]
        return (F(0.114) * b + F(0.587) * g) + F(0.299) * r

    def padded_size(self):
        """:233-236 -> (padded_height, padded_width)"""
        tw, th = self.target_size
        m = F(self.padding_multiple)
        up = lambda v: int(F(np.ceil(F(F(v) / m)) * m))
        return up(th), up(tw)

    def preprocess_batch(self, images: Sequence[np.ndarray]) -> np.ndarray:
        """:63-74 -> [n, 1, Hp, Wp] f32, 1.0 outside the target rectangle"""
        tw, th = self.target_size
        ph, pw = self.padded_size()
        t = np.full((len(images), 1, ph, pw), 1.0, np.float32)
        for i, img in enumerate(images):
            img = np.ascontiguousarray(img, np.uint8)
            t[i, 0, :th, :tw] = self.normalize_and_to_grayscale(self.resize_and_pad(self.crop_margin(img)))
        return t


class UniMERNetPreprocessor:
    """unimernet_preprocess.rs:43-281.  target_size is (width, height), as in the reference.  Other than FormulaPreprocessor: the margin crop has no
    `min_x >= max_x` fall-back (a single dark pixel crops to 1 x 1), the resize brings the SMALLER side to min(target) and shrinks a second time only when a side
    still exceeds the target, the canvas is white, grey comes before the normalisation, and the tensor is exactly the padded target."""

    def __init__(self, target_size=(672, 192), crop_threshold: int = 200, padding_multiple: int = 32, normalize_mean=(0.7931, 0.7931, 0.7931),
                 normalize_std=(0.1738, 0.1738, 0.1738)):
        self.target_size = (int(target_size[0]), int(target_size[1]))
        self.crop_threshold = int(crop_threshold)
        self.padding_multiple = int(padding_multiple)
        self.mean = np.asarray(normalize_mean, np.float32)
        self.std = np.asarray(normalize_std, np.float32)

    def crop_rect(self, img: np.ndarray):
        """:50-121 -> (x, y, w, h) of the inclusive foreground box, or None where the reference returns the image as it is"""
        gray = to_luma8(img)
        if gray.size == 0:
            return None
        mn, mx = gray.min(), gray.max()
        if mx == mn:                                                                               # :69
            return None
        norm = _as_u8((gray.astype(np.float32) - F(mn)) / F(F(mx) - F(mn)) * F(255.0))            # :78-80
        ys, xs = np.nonzero(norm < self.crop_threshold)
        if ys.size == 0:                                                                           # :114
            return None
        x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
        return x0, y0, x1 - x0 + 1, y1 - y0 + 1                                                    # :119

    def crop_margin(self, img: np.ndarray) -> np.ndarray:
        r = self.crop_rect(img)
        if r is None:
            return img
        x, y, w, h = r
        return np.ascontiguousarray(img[y:y + h, x:x + w])

    def resized_sizes(self, w: int, h: int):
        """:125-158 -> ((new_width, new_height), (final_width, final_height) or None): f32 scales, truncating casts; the second resize only when the first
        leaves a side above the target"""
        tw, th = self.target_size
        scale = F(F(min(tw, th)) / F(w if w <= h else h))
        nw, nh = _as_u32(F(F(w) * scale)), _as_u32(F(F(h) * scale))
        if not (nw > tw or nh > th):
            return (nw, nh), None
        s2 = min(F(F(tw) / F(nw)), F(F(th) / F(nh)))
        return (nw, nh), (_as_u32(F(F(nw) * s2)), _as_u32(F(F(nh) * s2)))

    @staticmethod
    def _resize(img: np.ndarray, nw: int, nh: int) -> np.ndarray:
        h, w = img.shape[:2]
        if (nw, nh) == (w, h):                         # (a Triangle resize to the same size is the identity)
            return img[..., :3]
        if w == 1 and h == 1:                          # (one source pixel: every output pixel is that pixel, whatever the filter)
            return np.broadcast_to(img[0, 0, :3], (nh, nw, 3)).copy()
        return api.k_resize_triangle(img, nw, nh)

    def resize_unimernet(self, img: np.ndarray):
        """:125-161 -> RGB, or None when a side is or truncates to 0 (what the image crate does then is not pinned: the canvas stays white)"""
        h, w = img.shape[:2]
        if w == 0 or h == 0:
            return None
        for size in self.resized_sizes(w, h):
            if size is None:
                break
            if size[0] == 0 or size[1] == 0:
                return None
            img = self._resize(np.ascontiguousarray(img), size[0], size[1])
        return img

    def add_padding(self, img) -> np.ndarray:
        """:164-188 -> RGB [th, tw, 3], the image centred on white (delta // 2 left and top)"""
        tw, th = self.target_size
        out = np.full((th, tw, 3), 255, np.uint8)
        if img is None:
            return out
        h, w = img.shape[:2]
        left, top = max(tw - w, 0) // 2, max(th - h, 0) // 2
        hh, ww = min(h, th - top), min(w, tw - left)                                               # :182
        out[top:top + hh, left:left + ww] = img[:hh, :ww, :3]
        return out

    def padded_size(self):
        """:209-211 -> (padded_height, padded_width)"""
        tw, th = self.target_size
        m = self.padding_multiple
        return -(-th // m) * m, -(-tw // m) * m

    def border_value(self) -> np.float32:
        """:235-236 the normalised white that fills the tensor outside the image"""
        return F(F(F(1.0) - self.mean[0]) / self.std[0])

    def image_to_tensor(self, img: np.ndarray) -> np.ndarray:
        """:205-249 -> [Hp, Wp] f32: grey = (0.299 r + 0.587 g + 0.114 b) / 255 summed left to right, then (grey - mean[0]) / std[0]"""
        h, w = img.shape[:2]
        ph, pw = self.padded_size()
        t = np.full((ph, pw), self.border_value(), np.float32)
        c = np.asarray(img, np.uint8).astype(np.float32)
        grey = ((F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2]) / F(255.0)
        t[:h, :w] = (grey - self.mean[0]) / self.std[0]
        return t

    def preprocess_single(self, img: np.ndarray) -> np.ndarray:
        """:191-202 -> RGB [th, tw, 3]"""
        return self.add_padding(self.resize_unimernet(self.crop_margin(np.ascontiguousarray(img, np.uint8))))

    def preprocess_batch(self, images: Sequence[np.ndarray]) -> np.ndarray:
        """:252-280 -> [n, 1, Hp, Wp] f32"""
        if len(images) == 0:
            raise api.OCRError(api.OAR_INVALID_INPUT, "invalid input: Empty image batch")
        return np.stack([self.image_to_tensor(self.preprocess_single(img)) for img in images])[:, None]


# ------------------------------------------------------------------------------------------------ tokens
def filter_tokens(token_ids, sos_token_id: int = 0, eos_token_id: int = 2, vocab_size: int = 2 ** 63 - 1) -> List[List[int]]:
    """PPFormulaNetModel::filter_tokens (pp_formulanet.rs:215-241): per row, stop at eos, then at the first non-negative id >= vocab_size (the sentinel some
    exports pad with); negative ids and sos are dropped without stopping."""
    out = []
    for row in np.asarray(token_ids, np.int64).reshape(len(token_ids), -1):
        toks = []
        for t in row.tolist():
            if t == eos_token_id:
                break
            if not (t < 0 or t < vocab_size):
                break
            if t >= 0 and t != sos_token_id:
                toks.append(t)
        out.append(toks)
    return out


def _bytes_to_unicode() -> Dict[int, str]:
    """the GPT-2 byte <-> printable character table of the ByteLevel pre-tokenizer / decoder"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


_CHAR_TO_BYTE = {c: b for b, c in _bytes_to_unicode().items()}

BOS_CANDIDATES = ("<s>", "[BOS]", "<bos>", "[CLS]")      # formula_recognition_adapter.rs:48-82
EOS_CANDIDATES = ("</s>", "[EOS]", "<eos>", "[SEP]")


class FormulaTokenizer:
    """The part of a Hugging Face `tokenizer.json` that decoding needs: `model.vocab`, `added_tokens` and a ByteLevel decoder."""

    def __init__(self, spec: dict):
        dec = spec.get("decoder") or {}
        kind = dec.get("type")
        if kind != "ByteLevel":
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: tokenizer decoder '{kind}' is not supported: only ByteLevel is")
        vocab = (spec.get("model") or {}).get("vocab")
        if not isinstance(vocab, dict):
            raise api.OCRError(api.OAR_INVALID_INPUT, "invalid input: tokenizer.json has no model.vocab table")
        self._vocab = {str(k): int(v) for k, v in vocab.items()}
        self._id_to_token = {v: k for k, v in self._vocab.items()}
        self._added, self._special = {}, set()
        for a in spec.get("added_tokens") or []:
            self._added[str(a["content"])] = int(a["id"])
            self._id_to_token[int(a["id"])] = str(a["content"])
            if a.get("special"):
                self._special.add(int(a["id"]))

    @classmethod
    def from_file(cls, path) -> "FormulaTokenizer":
        try:
            with open(path, "r", encoding="utf-8") as f:
                spec = json.load(f)
        except (OSError, ValueError) as e:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: Failed to load tokenizer from {str(path)!r}: {e}")
        return cls(spec)

    def token_to_id(self, token: str) -> Optional[int]:
        if token in self._added:
            return self._added[token]
        return self._vocab.get(token)

    def vocab_size(self, with_added: bool = True) -> int:
        n = len(self._vocab)
        return n + sum(1 for t in self._added if t not in self._vocab) if with_added else n

    def decode(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        """the token strings concatenated, mapped back through the byte table, decoded as UTF-8 with replacement characters"""
        text = "".join(self._id_to_token[i] for i in ids if i in self._id_to_token and not (skip_special_tokens and i in self._special))
        raw = bytearray()
        for ch in text:
            b = _CHAR_TO_BYTE.get(ch)
            raw += bytes([b]) if b is not None else ch.encode("utf-8")      # (a character outside the table: kept as it is)
        return raw.decode("utf-8", errors="replace")

    def special_token_ids(self):
        """extract_special_token_ids -> (sos, eos): the first candidate the tokenizer knows, else 0 / 2"""
        first = lambda names, default: next((i for i in (self.token_to_id(n) for n in names) if i is not None), default)
        return first(BOS_CANDIDATES, 0), first(EOS_CANDIDATES, 2)


# ------------------------------------------------------------------------------------------------ LaTeX clean-up
_WS = "\t\n\x0b\x0c\r \x85\xa0                　"     # Unicode White_Space (Rust char::is_whitespace, regex \s)
_WSC = "[" + re.escape(_WS) + "]"
_CHINESE_TEXT = re.compile(r"\\text" + _WSC + r"*\{([^{}]*[一-鿿]+[^{}]*)\}")
_TEXT_COMMAND = re.compile(r"(\\(operatorname|mathrm|text|mathbf)" + _WSC + r"?\*?" + _WSC + r"*\{.*?\})")
_LETTER_TO_NONLETTER = re.compile(r"([a-zA-Z])" + _WSC + r"+([^a-zA-Z])")


def _is_letter(c: str) -> bool:
    return ("a" <= c <= "z") or ("A" <= c <= "Z")


def normalize_latex(latex: str) -> str:
    """formula_preprocess.rs:268-372, statement for statement."""
    result = _CHINESE_TEXT.sub(lambda m: m.group(1), latex)                      # :272
    result = result.replace('"', "")                                             # :273
    result = _TEXT_COMMAND.sub(lambda m: m.group(0).replace(" ", ""), result)    # :279-295
    prev, iterations = None, 0
    while prev != result and iterations < 10:                                    # :306
        prev = result
        chars, out, i, n = result, [], 0, len(result)
        while i < n:                                                             # :320-359
            if i + 1 < n and chars[i] == "\\" and chars[i + 1] == " ":           # the LaTeX thin space `\ `: the backslash starts no match
                out.append(chars[i])
                i += 1
            elif i + 1 < n and chars[i + 1] in _WS:
                j = i + 1
                while j < n and chars[j] in _WS:
                    j += 1
                if j < n and not _is_letter(chars[i]):                           # non-letter, spaces, anything: the spaces go
                    out.append(chars[i])
                    i = j
                else:
                    out.append(chars[i])
                    i += 1
            else:
                out.append(chars[i])
                i += 1
        result = _LETTER_TO_NONLETTER.sub(lambda m: m.group(1) + m.group(2), "".join(out))     # :364-366
        iterations += 1
    return result.strip(_WS)                                                     # :371


# ------------------------------------------------------------------------------------------------ the predictor
class FormulaRecognitionPredictor:
    """FormulaRecognitionAdapter::execute (:170-286) over PPFormulaNetModel: batches of `batch_size` crops -> FormulaPreprocessor -> the graph through the engine
    -> the unique 2-D int64 output -> filter_tokens -> truncation to max_length -> tokenizer decode -> normalize_latex.  A formula in which an id at or above
    the tokenizer's vocabulary size survives the filter comes back as an empty string.  The preprocessor's target size is the model's input size when the
    file declares it (pp_formulanet.rs:340-353).

    stop_at_eos: the decode ends a chunk of 16 images once every one of them has emitted the tokenizer's eos instead of running all `M` steps of the Loop.
    `predict` and `decode` give the same strings either way (the filter stops at a row's first eos; only ids after it differ: they read eos), and `M` is of the
    order of 1536 where a formula has a few dozen to a few hundred tokens, so real use wants it on.  The default is off: `infer` then returns exactly what the
    graph's Loop computes.

    model_type: "pp_formulanet" (the default) or "unimernet" (formula_recognition_adapter.rs builds either).  "unimernet" selects UniMERNetPreprocessor and its
    default target (672, 192), takes the graph's FIRST output as the token ids (unimernet.rs:137-151) and makes the messages say `UniMERNet:`; the tokenizer,
    the token filter, normalize_latex and stop_at_eos are shared."""

    MODEL_TYPES = {"pp_formulanet": ("PP-FormulaNet", (384, 384)), "unimernet": ("UniMERNet", (672, 192))}

    def __init__(self, model: bytes, tokenizer, config: Optional[FormulaRecognitionConfig] = None, target_size: Optional[tuple] = None, device_id: int = 0,
                 stop_at_eos: bool = False, model_type: str = "pp_formulanet"):
        if model_type not in self.MODEL_TYPES:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: unknown formula model type {model_type!r}: expected one of {sorted(self.MODEL_TYPES)}")
        self.model_type = model_type
        self.model_name, default_size = self.MODEL_TYPES[model_type]
        self.config = config or FormulaRecognitionConfig()
        self.tokenizer = tokenizer if isinstance(tokenizer, FormulaTokenizer) else FormulaTokenizer.from_file(tokenizer)
        self.sos_token_id, self.eos_token_id = self.tokenizer.special_token_ids()
        self._eng = api.OrtInfer(model, device_id=device_id)
        self.stop_at_eos = bool(stop_at_eos)
        if self.stop_at_eos:
            self._eng.set_decode_stop(self.eos_token_id)
        size = default_size if target_size is None else (int(target_size[0]), int(target_size[1]))
        if size == default_size:                       # (pp_formulanet.rs:340-353, unimernet.rs:280-290)
            dims = self._eng.primary_input_shape()
            if dims is not None and len(dims) >= 4 and dims[-2] > 0 and dims[-1] > 0:
                size = (int(dims[-1]), int(dims[-2]))
        self.preprocessor = UniMERNetPreprocessor(target_size=size) if model_type == "unimernet" else FormulaPreprocessor(target_size=size)

    def recommended_batch_size(self) -> int:
        return self.config.batch_size

    def infer(self, batch: np.ndarray) -> np.ndarray:
        """pp_formulanet.rs:117-186, unimernet.rs:118-152 -> token ids [n, T] int64"""
        outs = self._eng.infer(batch)
        if self.model_type == "unimernet":
            if not outs:
                raise api.OCRError(api.OAR_INVALID_INPUT, "invalid input: UniMERNet: no output returned from inference")
            name, a = outs[0]
            if a.dtype != np.int64 or a.ndim != 2:
                raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: UniMERNet: failed to convert output to 2D i64 array: the first output '{name}' is {a.dtype} {list(a.shape)}")
            return a
        ids = [a for _, a in outs if a.dtype == np.int64 and a.ndim == 2]
        if len(ids) != 1:
            seen = [(n, str(a.dtype), list(a.shape)) for n, a in outs]
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: PP-FormulaNet: expected exactly one 2-D i64 output (token ids); found {len(ids)} candidate(s) among outputs {seen}")
        return ids[0]

    def decode_stats(self) -> "api.DecodeStats":
        """steps of the last `infer`: the Loop's limit, what the host enqueued and what did work on the device"""
        return self._eng.decode_stats()

    def decode(self, token_ids: np.ndarray, config: Optional[FormulaRecognitionConfig] = None) -> List[str]:
        cfg = config or self.config
        vocab = self.tokenizer.vocab_size(True)
        formulas = []
        for toks in filter_tokens(token_ids, self.sos_token_id, self.eos_token_id, vocab):
            toks = toks[:cfg.max_length]
            if toks and max(toks) >= vocab:
                formulas.append("")
                continue
            formulas.append(normalize_latex(self.tokenizer.decode(toks, True)))
        return formulas

    def predict(self, images: Sequence[np.ndarray], config: Optional[FormulaRecognitionConfig] = None) -> FormulaRecognitionOutput:
        cfg = config or self.config
        out = FormulaRecognitionOutput()
        bs = max(int(cfg.batch_size), 1)
        for i0 in range(0, len(images), bs):
            formulas = self.decode(self.infer(self.preprocessor.preprocess_batch(images[i0:i0 + bs])), cfg)
            out.formulas.extend(formulas)
            out.scores.extend([None] * len(formulas))
        return out

    def close(self):
        if getattr(self, "_eng", None) is not None:
            self._eng.close()
            self._eng = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
