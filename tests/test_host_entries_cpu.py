"""Bad calls of the host entries answer with a fixed status and a fixed text (tests/golden/host_entry_errors.json).

Every call listed here is refused before the entry asks for the device, so it answers the same with and without a GPU: a null buffer, each documented range
or alignment refusal, an output that does not fit, and pairs of faults whose first refusal pins the order of the checks.  The model entries get a missing
tensor, a wrong shape, a wrong dtype and a null argument.  One valid call per entry ("valid") reaches the device check: without a GPU it must give OAR_DEVICE
and the "no HIP device visible" text, and it is not made where a GPU is present.  The model entries' valid call carries device id -1, which a machine with a
GPU refuses with the entry's own "no such device".

The fixture is what `python tests/test_host_entries_cpu.py` writes: it was recorded before the host entries were moved onto their shared layer
(csrc/host_entry.h) and is replayed unchanged; the rows of the five image entries of DESIGN 4.53 were added with those entries."""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api, vl  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "host_entry_errors.json"
NO_DEVICE = "no HIP device visible: libOarMi355x has no CPU fallback"

_f = np.zeros(1 << 14, np.float32)
_i = np.zeros(64, np.int32)
_one = np.ones(64, np.int32)
_u8 = np.zeros(4096, np.uint8)
_ptrs = (C.c_void_p * 16)(*[_i.ctypes.data] * 16)
_out32 = (C.c_uint32 * 2)()
SYM = {"F": _f.ctypes.data, "I": _i.ctypes.data, "ONE": _one.ctypes.data, "U8": _u8.ctypes.data, "PP": C.cast(_ptrs, C.c_void_p).value, "NULL": None}


def _lens(*v):
    a = np.asarray(v, np.int32)
    SYM[f"L{len(SYM)}"] = a.ctypes.data
    _lens.keep.append(a)
    return f"L{len(SYM) - 1}"


_lens.keep = []
SEG_33_5, SEG_EMPTY, GRID_2x3, GRID_BAD, ROWS_OUT, IDX_OUT = _lens(33, 5), _lens(33, 0), _lens(2, 3), _lens(0, 3), _lens(5, 0), _lens(0, 9)
# the image entries of DESIGN 4.53: 64 images of 4 x 4 (all the same bytes), their widths, channel orders, two page offsets, room for the outputs
PU8, W4, W0 = (C.c_void_p * 64)(*[_u8.ctypes.data] * 64), (C.c_uint32 * 64)(*[4] * 64), (C.c_uint32 * 64)()
SRC_012, SRC_BAD = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 3)(0, 3, 2)
_offs, _out64, _cnt, _tensors = np.asarray([0, 49], np.uint64), (C.c_size_t * 2)(), (C.c_int32 * 2)(), (api.Tensor * 16)()
OFF_PAGES, FP, N_OUT, TENSORS = _offs.ctypes.data, _f.ctypes.data_as(C.POINTER(C.c_float)), C.cast(_cnt, C.POINTER(C.c_int32)), C.cast(_tensors, C.POINTER(api.Tensor))

# entry -> (parameter names, a valid call, [(label, overrides)]); a string value names a buffer of SYM, anything else goes to ctypes as it is
DIRECT = {
    "oar_k_mha_attention": (
        "buf buf_floats q_off k_off v_off ldq ldk ldv n tq tk heads head_dim scale scale_pre o_io o_floats o_off".split(),
        dict(buf="F", buf_floats=4096, q_off=0, k_off=1024, v_off=2048, ldq=16, ldk=16, ldv=16, n=1, tq=5, tk=7, heads=2, head_dim=8, scale=0.35, scale_pre=0, o_io="F", o_floats=256, o_off=0),
        [("null buf", dict(buf="NULL")), ("null o_io", dict(o_io="NULL")), ("shape", dict(heads=0)), ("head_dim", dict(head_dim=7)), ("stride below D", dict(ldq=8)),
         ("stride no multiple of 4", dict(ldk=18)), ("offset alignment", dict(q_off=2)), ("view does not fit", dict(v_off=4088)), ("output does not fit", dict(o_floats=79)),
         ("output offset past the end", dict(o_off=260)), ("null before shape", dict(buf="NULL", heads=0)), ("shape before stride", dict(heads=0, ldq=8)),
         ("stride before alignment", dict(ldq=8, q_off=2)), ("alignment before fit", dict(o_off=2, o_floats=1)), ("view before output", dict(v_off=4088, o_floats=1))]),
    "oar_k_vis_attention": (
        "buf buf_floats qkv_off ld seg_lens n_segs heads head_dim cos_tab sin_tab o_io o_floats o_off".split(),
        dict(buf="F", buf_floats=38 * 48, qkv_off=0, ld=48, seg_lens=SEG_33_5, n_segs=2, heads=2, head_dim=8, cos_tab="F", sin_tab="F", o_io="F", o_floats=38 * 16, o_off=0),
        [("null buf", dict(buf="NULL")), ("null seg_lens", dict(seg_lens="NULL")), ("null cos", dict(cos_tab="NULL")), ("heads", dict(heads=0)), ("head_dim", dict(head_dim=12)),
         ("n_segs", dict(n_segs=0)), ("empty segment", dict(seg_lens=SEG_EMPTY)), ("stride", dict(ld=44)), ("offset alignment", dict(o_off=1)),
         ("qkv does not fit", dict(buf_floats=38 * 48 - 1)), ("output does not fit", dict(o_floats=38 * 16 - 1)), ("null before heads", dict(o_io="NULL", heads=0)),
         ("heads before head_dim", dict(heads=0, head_dim=12)), ("segment before stride", dict(seg_lens=SEG_EMPTY, ld=44)), ("qkv before output", dict(buf_floats=1, o_floats=1))]),
    "oar_k_vis_pos_embed": (
        "table pos_grid hidden grids n_images o_io o_floats o_off".split(),
        dict(table="F", pos_grid=4, hidden=8, grids=GRID_2x3, n_images=1, o_io="F", o_floats=48, o_off=0),
        [("null table", dict(table="NULL")), ("null grids", dict(grids="NULL")), ("pos_grid", dict(pos_grid=0)), ("hidden", dict(hidden=6)), ("n_images", dict(n_images=17)),
         ("offset alignment", dict(o_off=2)), ("grid side", dict(grids=GRID_BAD)), ("output does not fit", dict(o_floats=47)), ("null before range", dict(o_io="NULL", hidden=6)),
         ("alignment before grid", dict(o_off=2, grids=GRID_BAD)), ("grid before fit", dict(grids=GRID_BAD, o_floats=1))]),
    "oar_k_add_layernorm": (
        "a b b_rows gamma beta rows C eps write_sum o_io o_floats y_off s_off".split(),
        dict(a="F", b="F", b_rows=3, gamma="F", beta="F", rows=3, C=8, eps=1e-5, write_sum=1, o_io="F", o_floats=48, y_off=0, s_off=24),
        [("null a", dict(a="NULL")), ("null o_io", dict(o_io="NULL")), ("rows", dict(rows=0)), ("b_rows does not divide", dict(b_rows=2)), ("eps", dict(eps=0.0)),
         ("y does not fit", dict(y_off=25)), ("sum does not fit", dict(s_off=25)), ("overlap", dict(s_off=8)), ("null before rows", dict(b="NULL", rows=0)),
         ("rows before eps", dict(C=0, eps=0.0)), ("y before sum", dict(y_off=40, s_off=40)), ("eps before fit", dict(eps=-1.0, o_floats=1))]),
    "oar_k_relpos_attention": (
        "qkv b h w ws heads head_dim rh rw bqkv scale scale_pre o_io o_floats o_off".split(),
        dict(qkv="F", b=1, h=3, w=5, ws=0, heads=2, head_dim=8, rh="F", rw="F", bqkv="NULL", scale=0.35, scale_pre=0, o_io="F", o_floats=240, o_off=0),
        [("null qkv", dict(qkv="NULL")), ("null table", dict(rw="NULL")), ("shape", dict(heads=0)), ("offset alignment", dict(o_off=3)), ("output does not fit", dict(o_floats=239)),
         ("null before shape", dict(o_io="NULL", heads=0)), ("shape before alignment", dict(b=0, o_off=3)), ("alignment before fit", dict(o_off=2, o_floats=1))]),
    "oar_k_lm_gemm": (
        "x m k w w_dtype n o_io o_floats o_off".split(),
        dict(x="F", m=3, k=8, w="F", w_dtype=1, n=5, o_io="F", o_floats=15, o_off=0),
        [("null x", dict(x="NULL")), ("null w", dict(w="NULL")), ("dtype", dict(w_dtype=2)), ("m", dict(m=0)), ("k multiple of 4", dict(k=6)), ("output does not fit", dict(o_floats=14)),
         ("offset past the end", dict(o_off=16)), ("null before dtype", dict(o_io="NULL", w_dtype=2)), ("dtype before m", dict(w_dtype=2, m=0)), ("range before multiple", dict(n=0, k=6)),
         ("multiple before fit", dict(k=6, o_floats=1))]),
    "oar_k_lm_prefill_attention": (
        "q kcache vcache n_seq max_positions starts lens heads kv_heads head_dim o_io o_floats o_off".split(),
        dict(q="F", kcache="F", vcache="F", n_seq=2, max_positions=40, starts="I", lens=SEG_33_5, heads=2, kv_heads=1, head_dim=8, o_io="F", o_floats=38 * 16, o_off=0),
        [("null q", dict(q="NULL")), ("null lens", dict(lens="NULL")), ("heads", dict(heads=3, kv_heads=2)), ("head_dim", dict(head_dim=6)), ("n_seq", dict(n_seq=0)),
         ("empty sequence", dict(lens=SEG_EMPTY)), ("positions outside the cache", dict(max_positions=32)), ("offset alignment", dict(o_off=1)), ("output does not fit", dict(o_floats=38 * 16 - 1)),
         ("null before heads", dict(o_io="NULL", heads=0)), ("heads before head_dim", dict(heads=0, head_dim=6)), ("sequence before alignment", dict(lens=SEG_EMPTY, o_off=1)),
         ("alignment before fit", dict(o_off=2, o_floats=1))]),
    "oar_k_lm_decode_attention": (
        "q kcache vcache n_seq max_positions n_rows row_seq row_pos heads kv_heads head_dim split_keys o_io o_floats o_off".split(),
        dict(q="F", kcache="F", vcache="F", n_seq=2, max_positions=40, n_rows=2, row_seq="I", row_pos="I", heads=2, kv_heads=1, head_dim=8, split_keys=0, o_io="F", o_floats=32, o_off=0),
        [("null q", dict(q="NULL")), ("null row_pos", dict(row_pos="NULL")), ("heads", dict(kv_heads=0)), ("head_dim", dict(head_dim=132)), ("max_positions", dict(max_positions=0)),
         ("n_rows", dict(n_rows=17)), ("split_keys", dict(split_keys=65)), ("row outside", dict(row_seq=ROWS_OUT)), ("offset alignment", dict(o_off=2)), ("output does not fit", dict(o_floats=31)),
         ("null before heads", dict(vcache="NULL", kv_heads=0)), ("n_rows before split_keys", dict(n_rows=0, split_keys=65)), ("row before alignment", dict(row_seq=ROWS_OUT, o_off=2)),
         ("alignment before fit", dict(o_off=2, o_floats=1))]),
    "oar_k_lm_select": (
        "logits n_rows vocab hist_lengths hist_ids repetition_penalty no_repeat_ngram_size tokens_io n_tokens off".split(),
        dict(logits="F", n_rows=2, vocab=9, hist_lengths="ONE", hist_ids="PP", repetition_penalty=1.5, no_repeat_ngram_size=2, tokens_io="I", n_tokens=2, off=0),
        [("null logits", dict(logits="NULL")), ("null hist_ids", dict(hist_ids="NULL")), ("n_rows", dict(n_rows=0)), ("vocab", dict(vocab=1)), ("penalty", dict(repetition_penalty=0.5)),
         ("ngram", dict(no_repeat_ngram_size=-1)), ("ngram with a large vocabulary", dict(vocab=(1 << 19) + 1)), ("tokens do not fit", dict(n_tokens=1)), ("offset past the end", dict(off=3)),
         ("null before n_rows", dict(tokens_io="NULL", n_rows=0)), ("n_rows before vocab", dict(n_rows=0, vocab=1)), ("penalty before fit", dict(repetition_penalty=0.5, n_tokens=1))]),
    "oar_k_qvis_rmsnorm": (
        "x g rows d eps o_io o_floats o_off".split(),
        dict(x="F", g="F", rows=3, d=8, eps=1e-6, o_io="F", o_floats=24, o_off=0),
        [("null x", dict(x="NULL")), ("null o_io", dict(o_io="NULL")), ("rows", dict(rows=0)), ("d", dict(d=6)), ("eps", dict(eps=-1.0)), ("offset alignment", dict(o_off=2)),
         ("output does not fit", dict(o_floats=23)), ("null before rows", dict(g="NULL", rows=0)), ("range before fit", dict(d=6, o_floats=1))]),
    "oar_k_qvis_act": (
        "in_ in_floats rows f act gated o_io o_floats o_off".split(),
        dict(in_="F", in_floats=48, rows=3, f=8, act=1, gated=1, o_io="F", o_floats=24, o_off=0),
        [("null in", dict(in_="NULL")), ("rows", dict(rows=0)), ("f", dict(f=6)), ("activation", dict(act=9)), ("input too short", dict(in_floats=47)), ("offset alignment", dict(o_off=1)),
         ("output does not fit", dict(o_floats=23)), ("null before rows", dict(o_io="NULL", rows=0)), ("range before activation", dict(f=6, act=9)), ("activation before input", dict(act=9, in_floats=1)),
         ("input before output", dict(in_floats=1, o_floats=1))]),
    "oar_k_qvis_row_gather": (
        "in_ n_in_rows row_floats idx n_rows o_io o_floats o_off".split(),
        dict(in_="F", n_in_rows=5, row_floats=8, idx="I", n_rows=2, o_io="F", o_floats=16, o_off=0),
        [("null in", dict(in_="NULL")), ("null idx", dict(idx="NULL")), ("row counts", dict(n_rows=0)), ("row_floats", dict(row_floats=6)), ("index outside", dict(idx=IDX_OUT)),
         ("offset alignment", dict(o_off=2)), ("output does not fit", dict(o_floats=15)), ("null before rows", dict(o_io="NULL", n_rows=0)), ("range before index", dict(row_floats=6, idx=IDX_OUT)),
         ("index before fit", dict(idx=IDX_OUT, o_floats=1))]),
    # the image kernels: one check of their arguments, then the device
    "oar_k_normalize": ("rgb w h src_channels alpha beta hwc_layout out".split(), dict(rgb="U8", w=4, h=4, src_channels=_i.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                                     alpha=_f.ctypes.data_as(C.POINTER(C.c_float)), beta=_f.ctypes.data_as(C.POINTER(C.c_float)), hwc_layout=0, out="F"),
                        [("null rgb", dict(rgb="NULL")), ("null out", dict(out="NULL"))]),
    "oar_k_resize_triangle": ("rgb w h nw nh out".split(), dict(rgb="U8", w=4, h=4, nw=3, nh=5, out="U8"), [("null rgb", dict(rgb="NULL")), ("zero width", dict(nw=0))]),
    "oar_k_resize_filter": ("rgb w h nw nh filter out".split(), dict(rgb="U8", w=4, h=4, nw=3, nh=5, filter=1, out="U8"),
                            [("null out", dict(out="NULL")), ("zero height", dict(h=0)), ("filter", dict(filter=3))]),
    "oar_k_threshold": ("pred n thresh mask".split(), dict(pred="F", n=16, thresh=0.3, mask="U8"), [("null pred", dict(pred="NULL")), ("null mask", dict(mask="NULL"))]),
    "oar_k_dilate": ("mask height width out".split(), dict(mask="U8", height=4, width=4, out="U8"), [("null mask", dict(mask="NULL")), ("zero width", dict(width=0))]),
    "oar_k_poly_scores": ("pred height width pts_xy counts n_polys scores".split(), dict(pred="F", height=4, width=4, pts_xy="F", counts=_i.ctypes.data_as(C.POINTER(C.c_uint32)), n_polys=1, scores="F"),
                          [("null pred", dict(pred="NULL")), ("null scores", dict(scores="NULL")), ("zero height", dict(height=0))]),
    "oar_k_rotate_rgb": ("rgb w h quarter out".split(), dict(rgb="U8", w=4, h=4, quarter=1, out="U8"), [("null rgb", dict(rgb="NULL")), ("quarter", dict(quarter=4))]),
    "oar_k_bgr_planes_to_rgb": ("planes plane scale out".split(), dict(planes="F", plane=16, scale=255.0, out="U8"), [("null planes", dict(planes="NULL")), ("null out", dict(out="NULL"))]),
    "oar_k_rotate_crop": ("rgb w h box out cap out_w out_h".split(), dict(rgb="U8", w=4, h=4, box=_f.ctypes.data_as(C.POINTER(C.c_float)), out="U8", cap=4096,
                                                                       out_w=C.cast(_out32, C.POINTER(C.c_uint32)), out_h=C.cast(_out32, C.POINTER(C.c_uint32))),
                          [("null rgb", dict(rgb="NULL")), ("zero width", dict(w=0))]),
    # the u8 front kernels and the detector's finish kernels.  The stem's model bytes are not looked at before the device is: any bytes do here
    "oar_k_stem_u8": (
        "onnx onnx_len rgb widths n h wt src_channels alpha beta table outs max_out n_out".split(),
        dict(onnx="U8", onnx_len=64, rgb=PU8, widths=W4, n=2, h=4, wt=4, src_channels=SRC_012, alpha=FP, beta=FP, table=0, outs=TENSORS, max_out=16, n_out=N_OUT),
        [("null onnx", dict(onnx="NULL")), ("null outs", dict(outs="NULL")), ("no image", dict(n=0)), ("33 pages by value", dict(n=33)), ("wider than the tensor", dict(table=1, wt=3)),
         ("a page of another width", dict(wt=5)), ("source channel", dict(src_channels=SRC_BAD)), ("null before count", dict(rgb="NULL", n=33)),
         ("count before width", dict(n=33, wt=3)), ("width before channel", dict(table=1, wt=3, src_channels=SRC_BAD))]),
    "oar_k_rec_resize_u8": (
        "rgb widths heights flips n img_h img_w max_img_w sentinel tensor_width resized_widths pool pool_cap pool_bytes".split(),
        dict(rgb=PU8, widths=W4, heights=W4, flips="NULL", n=2, img_h=8, img_w=32, max_img_w=64, sentinel=0xA5, tensor_width=C.cast(_out32, C.POINTER(C.c_uint32)), resized_widths="I",
             pool="U8", pool_cap=4096, pool_bytes=C.cast(_out64, C.POINTER(C.c_size_t))),
        [("null rgb", dict(rgb="NULL")), ("null pool_bytes", dict(pool_bytes=None)), ("no crop", dict(n=0)), ("empty crop", dict(widths=W0)), ("pool too small", dict(pool_cap=64)),
         ("crop before pool", dict(widths=W0, pool_cap=64))]),
    "oar_k_normalize_pages": (
        "pool pool_bytes offsets n_pages plane src_channels alpha beta hwc_layout out".split(),
        dict(pool="U8", pool_bytes=4096, offsets=OFF_PAGES, n_pages=2, plane=16, src_channels=SRC_012, alpha=FP, beta=FP, hwc_layout=0, out="F"),
        [("null pool", dict(pool="NULL")), ("null out", dict(out="NULL")), ("no page", dict(n_pages=0)), ("33 pages", dict(n_pages=33)), ("page does not fit", dict(pool_bytes=96)),
         ("source channel", dict(src_channels=SRC_BAD)), ("count before fit", dict(n_pages=33, pool_bytes=1)), ("fit before channel", dict(pool_bytes=96, src_channels=SRC_BAD))]),
    "oar_k_db_keep_and_pack": (
        "net_out n channels height width thresh float_offset probs bits".split(),
        dict(net_out="F", n=2, channels=2, height=3, width=9, thresh=0.3, float_offset=1, probs="F", bits="U8"),
        [("null net_out", dict(net_out="NULL")), ("null bits", dict(bits="NULL")), ("zero width", dict(width=0)), ("float_offset", dict(float_offset=4)),
         ("null before offset", dict(probs="NULL", float_offset=4))]),
    "oar_k_pack_mask_bits": (
        "mask n height width byte_offset bits".split(),
        dict(mask="U8", n=2, height=3, width=9, byte_offset=3, bits="U8"),
        [("null mask", dict(mask="NULL")), ("zero height", dict(height=0)), ("byte_offset", dict(byte_offset=8)), ("null before offset", dict(bits="NULL", byte_offset=8))]),
}


def _bind():
    L = vl._lib()
    vl._vis_lib()
    vl._qvis_lib()
    for name, argtypes in (("oar_k_rotate_rgb", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p]), ("oar_k_bgr_planes_to_rgb", [C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]),
                           ("oar_k_resize_filter", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p])):
        fn = getattr(L, name)
        if fn.argtypes is None:
            fn.restype, fn.argtypes = C.c_int, argtypes
    return L


def _last_error(L):
    buf = C.create_string_buffer(4096)
    L.oar_last_error(buf, 4096)
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------- the model entries
def _table(shapes, drop=None, reshape=None, dtype=None):
    """name -> shape as an LmTensor array of float32 zeros; drop a name, give one another shape or another dtype code"""
    keep, rows = [], []
    for name, shape in shapes.items():
        if name == drop:
            continue
        a = np.zeros(reshape[1] if reshape and reshape[0] == name else shape, np.float32)
        e = vl.LmTensor()
        e.name, e.dtype, e.rank, e.data = name.encode(), (dtype[1] if dtype and dtype[0] == name else vl.OAR_LM_F32), a.ndim, a.ctypes.data
        for i, v in enumerate(a.shape):
            e.dims[i] = v
        keep.append(a)
        rows.append(e)
    return (vl.LmTensor * len(rows))(*rows), len(rows), keep


def _lm_cfg():
    return vl.CausalLMConfig(hidden_size=8, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1, head_dim=8, intermediate_size=8, vocab_size=4, mrope_section=(2, 1, 1),
                             max_positions=16, max_sequences=2).to_c()


def _lm_shapes():
    p = "model.layers.0."
    return {"model.embed_tokens.weight": (4, 8), "lm_head.weight": (4, 8), "model.norm.weight": (8,), p + "input_layernorm.weight": (8,), p + "post_attention_layernorm.weight": (8,),
            p + "self_attn.q_proj.weight": (8, 8), p + "self_attn.k_proj.weight": (8, 8), p + "self_attn.v_proj.weight": (8, 8), p + "self_attn.o_proj.weight": (8, 8),
            p + "mlp.gate_proj.weight": (8, 8), p + "mlp.up_proj.weight": (8, 8), p + "mlp.down_proj.weight": (8, 8)}


def _vis_cfg():
    return vl.VisionConfig(hidden_size=8, num_hidden_layers=1, num_attention_heads=1, intermediate_size=8, patch_size=2, text_hidden=8, pos_grid=3, max_tokens=16, max_images=2).to_c()


def _vis_shapes():
    v, p = "visual.vision_model.", "visual.vision_model.encoder.layers.0."
    s = {v + "embeddings.patch_embedding.weight": (8, 3, 2, 2), v + "embeddings.patch_embedding.bias": (8,), v + "embeddings.position_embedding.weight": (9, 8)}
    for n in ("layer_norm1", "layer_norm2"):
        s[p + n + ".weight"], s[p + n + ".bias"] = (8,), (8,)
    for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2"):
        s[p + n + ".weight"], s[p + n + ".bias"] = (8, 8), (8,)
    s.update({v + "post_layernorm.weight": (8,), v + "post_layernorm.bias": (8,), "mlp_AR.pre_norm.weight": (8,), "mlp_AR.pre_norm.bias": (8,), "mlp_AR.linear_1.weight": (32, 32),
              "mlp_AR.linear_1.bias": (32,), "mlp_AR.linear_2.weight": (8, 32), "mlp_AR.linear_2.bias": (8,)})
    return s


def _qvis_cfg(keep, **kw):
    d = dict(kind="qwen2", embed_dim=8, depth=1, num_heads=1, intermediate_size=8, patch_size=2, out_hidden_size=8, max_tokens=16, max_images=2)
    d.update(kw)
    return vl.QwenVisionConfig(**d).to_c(keep)


def _qvis_shapes():
    p = "blocks.0."
    s = {"patch_embed.proj.weight": (8, 24), p + "norm1.weight": (8,), p + "norm1.bias": (8,), p + "norm2.weight": (8,), p + "norm2.bias": (8,), p + "attn.qkv.weight": (24, 8),
         p + "attn.qkv.bias": (24,), p + "attn.proj.weight": (8, 8), p + "attn.proj.bias": (8,), p + "mlp.fc1.weight": (8, 8), p + "mlp.fc1.bias": (8,), p + "mlp.fc2.weight": (8, 8),
         p + "mlp.fc2.bias": (8,), "merger.ln_q.weight": (8,), "merger.ln_q.bias": (8,), "merger.mlp.0.weight": (32, 32), "merger.mlp.0.bias": (32,), "merger.mlp.2.weight": (8, 32),
         "merger.mlp.2.bias": (8,)}
    return s


def _lm_request(keep, **kw):
    ids = np.asarray([1, 2, 3], np.int32)
    lengths = np.asarray([3], np.int32)
    toks, counts = np.zeros(4, np.int32), np.zeros(1, np.int32)
    idp = (C.c_void_p * 1)(ids.ctypes.data)
    keep += [ids, lengths, toks, counts, idp]
    r = vl.LmRequest()
    r.n_seq, r.lengths, r.input_ids = 1, lengths.ctypes.data_as(C.POINTER(C.c_int32)), C.cast(idp, C.POINTER(C.c_void_p))
    r.max_new_tokens, r.eos_token_id, r.tokens, r.counts = 4, -1, toks.ctypes.data, counts.ctypes.data
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _create_cases(entry, fn, cfg_of, shapes, a_matrix, a_vector):
    """the five calls of a create entry; each returns the status"""
    def call(cfg, table, n, device=0):
        h = C.c_void_p()
        return fn(cfg, table, n, device, C.byref(h))

    def with_table(**kw):
        keep = []
        t, n, k2 = _table(shapes, **kw)
        keep.append(k2)
        return lambda device=0: call(C.byref(cfg_of(keep)), t, n, device)
    yield entry, "null cfg", lambda: call(None, None, 0)
    yield entry, "null out", lambda: fn(C.byref(cfg_of([])), None, 0, 0, None)
    yield entry, "missing tensor", with_table(drop=a_vector)
    yield entry, "wrong shape", with_table(reshape=(a_matrix, (3, 5)))
    yield entry, "wrong dtype", with_table(dtype=(a_vector, 7))
    yield entry, "two faults: the first tensor looked up", with_table(drop=a_matrix, dtype=(a_vector, 7))
    yield entry, "valid", lambda: with_table()(-1)


def _model_cases(L):
    yield from _create_cases("oar_lm_create", L.oar_lm_create, lambda keep: _lm_cfg(), _lm_shapes(), "model.layers.0.mlp.down_proj.weight", "model.norm.weight")
    yield from _create_cases("oar_vis_create", L.oar_vis_create, lambda keep: _vis_cfg(), _vis_shapes(), "mlp_AR.linear_2.weight", "visual.vision_model.post_layernorm.bias")
    yield from _create_cases("oar_qvis_create", L.oar_qvis_create, lambda keep: _qvis_cfg(keep), _qvis_shapes(), "merger.mlp.2.weight", "merger.ln_q.bias")

    def bad_lm_cfg():
        c = _lm_cfg()
        c.head_dim = 6
        return L.oar_lm_create(C.byref(c), None, 0, 0, C.byref(C.c_void_p()))
    yield "oar_lm_create", "head_dim", bad_lm_cfg
    f, b, n = C.c_double(), C.c_double(), C.c_int32()
    yield "oar_vis_cost", "null model", lambda: L.oar_vis_cost(None, 1, _i.ctypes.data, C.byref(f), C.byref(b), C.byref(n))
    yield "oar_qvis_cost", "null model", lambda: L.oar_qvis_cost(None, 1, _i.ctypes.data, C.byref(f), C.byref(b), C.byref(n))
    keep = []
    yield "oar_qvis_check", "null cfg", lambda: L.oar_qvis_check(None, 0, None)
    yield "oar_qvis_check", "heads", lambda: L.oar_qvis_check(C.byref(_qvis_cfg(keep, num_heads=3)), 0, None)
    yield "oar_qvis_check", "activation", lambda: L.oar_qvis_check(C.byref(vl.QwenVisionConfig(kind="qwen2", embed_dim=8, depth=1, num_heads=1, intermediate_size=8, patch_size=2,
                                                                                               out_hidden_size=8).to_c(keep, act=9)), 0, None)
    yield "oar_qvis_check", "null grids", lambda: L.oar_qvis_check(C.byref(_qvis_cfg(keep)), 1, None)
    g = np.asarray([3, 4], np.int32)
    yield "oar_qvis_check", "grid no multiple of merge", lambda: L.oar_qvis_check(C.byref(_qvis_cfg(keep)), 1, g.ctypes.data)
    big = np.asarray([8, 8], np.int32)
    yield "oar_qvis_check", "more patches than max_tokens", lambda: L.oar_qvis_check(C.byref(_qvis_cfg(keep)), 1, big.ctypes.data)
    yield "oar_qvis_check", "window size", lambda: L.oar_qvis_check(C.byref(_qvis_cfg(keep, kind="qwen2_5", window_size=0)), 0, None)
    yield "oar_lm_logits_check", "null cfg", lambda: L.oar_lm_logits_check(None, None, None)
    yield "oar_lm_logits_check", "n_seq", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, n_seq=3)), None)
    yield "oar_lm_logits_check", "max_new_tokens", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, max_new_tokens=0)), None)
    yield "oar_lm_logits_check", "null tokens", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, tokens=None)), None)
    yield "oar_lm_logits_check", "eos", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, eos_token_id=4)), None)
    yield "oar_lm_logits_check", "too long", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, max_new_tokens=14)), None)

    def processors(r, n, **kw):
        lp = vl.LmLogitsCfg()
        lp.repetition_penalty, lp.no_repeat_ngram_size = r, n
        for k, v in kw.items():
            setattr(lp, k, v)
        return L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep)), C.byref(lp))
    yield "oar_lm_logits_check", "penalty", lambda: processors(0.5, 0)
    yield "oar_lm_logits_check", "ngram", lambda: processors(1.0, -1)
    yield "oar_lm_logits_check", "history_ids without lengths", lambda: processors(1.5, 0, history_lengths=_i.ctypes.data)
    yield "oar_lm_logits_check", "request before processors", lambda: L.oar_lm_logits_check(C.byref(_lm_cfg()), C.byref(_lm_request(keep, max_new_tokens=0)), C.byref(vl.LmLogitsCfg()))


def _direct_cases(L):
    for entry, (names, valid, cases) in DIRECT.items():
        fn = getattr(L, entry)
        for label, over in [("valid", {})] + cases:
            args = dict(valid)
            args.update(over)
            argv = [SYM[args[n]] if isinstance(args[n], str) else args[n] for n in names]
            yield entry, label, (lambda fn=fn, argv=argv: fn(*argv))


def _all_cases(L):
    yield from _direct_cases(L)
    yield from _model_cases(L)


def record():
    """status and text of every call; the valid calls are left out (what they answer depends on the machine)"""
    L = _bind()
    out = []
    for entry, label, call in _all_cases(L):
        if label == "valid":
            continue
        st = int(call())
        out.append({"entry": entry, "call": label, "status": st, "error": _last_error(L)})
    return out


def test_every_entry_has_its_calls():
    """the fixture holds every call of this file, in order, and nothing else"""
    want = [(e, c) for e, c, _ in _all_cases(_bind()) if c != "valid"]
    got = [(r["entry"], r["call"]) for r in json.loads(GOLDEN.read_text())]
    assert got == want
    per_entry = {}
    for e, c in want:
        per_entry.setdefault(e, []).append(c)
    for entry in DIRECT:
        assert len(per_entry[entry]) >= 2, entry
    assert all(r["status"] not in (api.OAR_OK, api.OAR_DEVICE) and NO_DEVICE not in r["error"] for r in json.loads(GOLDEN.read_text()))   # refused before the device


@pytest.mark.parametrize("entry", sorted({e for e, _, _ in _all_cases(_bind())}))
def test_bad_calls_answer_as_recorded(entry):
    L = _bind()
    golden = {(r["entry"], r["call"]): r for r in json.loads(GOLDEN.read_text())}
    n = 0
    for e, label, call in _all_cases(L):
        if e != entry:
            continue
        if label == "valid":
            if api.device_count() == 0:
                st = int(call())
                assert (st, _last_error(L)) == (api.OAR_DEVICE, NO_DEVICE), (entry, label)
            elif entry.endswith("_create"):   # device id -1 on a machine with a GPU: the entry's own range check, nothing allocated
                st = int(call())
                assert (st, _last_error(L)) == (api.OAR_DEVICE, entry + ": no such device"), (entry, label)
            continue
        want = golden[(e, label)]
        st = int(call())
        assert (st, _last_error(L)) == (want["status"], want["error"]), (entry, label)
        n += 1
    assert n >= 1


if __name__ == "__main__":
    rows = record()
    bad = [r for r in rows if r["status"] in (api.OAR_OK, api.OAR_DEVICE)]
    assert not bad, f"these calls reach the device, they do not belong here: {bad}"
    GOLDEN.write_text(json.dumps(rows, indent=1) + "\n")
    print(f"{len(rows)} calls -> {GOLDEN}")
