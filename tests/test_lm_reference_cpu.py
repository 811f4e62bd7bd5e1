"""The torch-CPU reference of the decoder-only language model (synth/lm_reference.py) checked on its own, the conditions the GPU tests lean on (tolerance, greedy-safe
seeds), the safetensors reader, CausalLMConfig.from_hf_json and the argument checks of oar_lm_create that need no device."""
import json
import struct

import numpy as np
import pytest
import torch

from oar_ocr_amd import api, build, vl
from oar_ocr_amd.synth import lm_reference as R


def _full_forward(case, weights, x, pos3):
    """A second spelling of the model: the whole sequence at once, an explicit [T, T] mask, repeat_interleave for the kv heads, no cache, matmul / transposes in
    place of einsum, cos / sin gathered per channel.  -> logits [T, V] in f64."""
    w = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    T, H, KVH, dh = x.shape[0], case.heads, case.kv_heads, case.head_dim
    half = dh // 2
    inv = torch.tensor([case.theta ** (-(2.0 * i) / dh) for i in range(half)], dtype=torch.float64)
    axis_of = []
    for a, n in enumerate(case.mrope_section):
        axis_of += [a] * n
    axis_of = torch.tensor(axis_of + axis_of)                       # channel d of dh takes the positions of axis_of[d]
    freq_of = torch.cat([inv, inv])
    ang = pos3.double()[axis_of, :].T * freq_of[None, :]            # [T, dh]
    cos, sin = ang.cos(), ang.sin()

    def rms(v, g):
        return v / torch.sqrt(v.pow(2).sum(-1, keepdim=True) / v.shape[-1] + case.eps) * g

    def rope(v):                                                   # [T, n, dh]
        v1, v2 = v[..., :half], v[..., half:]
        return torch.cat([v1 * cos[:, None, :half] - v2 * sin[:, None, :half], v2 * cos[:, None, half:] + v1 * sin[:, None, half:]], dim=-1)

    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for l in range(case.L):
        p = f"model.layers.{l}."
        xn = rms(x, w[p + "input_layernorm.weight"])
        q, k, v = xn @ w[p + "self_attn.q_proj.weight"].T, xn @ w[p + "self_attn.k_proj.weight"].T, xn @ w[p + "self_attn.v_proj.weight"].T
        if case.qkv_bias:
            q, k, v = q + w[p + "self_attn.q_proj.bias"], k + w[p + "self_attn.k_proj.bias"], v + w[p + "self_attn.v_proj.bias"]
        q, k, v = rope(q.view(T, H, dh)), rope(k.view(T, KVH, dh)), v.view(T, KVH, dh)
        k, v = k.repeat_interleave(H // KVH, dim=1), v.repeat_interleave(H // KVH, dim=1)
        s = (q.transpose(0, 1) @ k.transpose(0, 1).transpose(1, 2)) / dh ** 0.5        # [H, T, T]
        s = torch.where(mask[None], s, torch.tensor(float("-inf"), dtype=torch.float64))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        a = e / e.sum(-1, keepdim=True)
        o = (a @ v.transpose(0, 1)).transpose(0, 1).reshape(T, H * dh)
        x = x + o @ w[p + "self_attn.o_proj.weight"].T
        xn = rms(x, w[p + "post_attention_layernorm.weight"])
        g, u = xn @ w[p + "mlp.gate_proj.weight"].T, xn @ w[p + "mlp.up_proj.weight"].T
        x = x + (g * torch.sigmoid(g) * u) @ w[p + "mlp.down_proj.weight"].T
    x = rms(x, w["model.norm.weight"])
    return x @ (w["model.embed_tokens.weight"] if case.tie else w["lm_head.weight"]).T


@pytest.mark.parametrize("name", list(R.CASES))
def test_cached_forward_equals_the_full_recomputation(name):
    """The step-by-step forward with its cache (prompt chunk, then one position at a time) against the uncached full-sequence forward over prompt + generated tokens."""
    _cached_equals_full(name, R.reference_for(name))


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_cached_forward_equals_the_full_recomputation_on_long_caches(name):
    _cached_equals_full(name, R.long_reference_for(name))


def _cached_equals_full(name, ref):
    case, weights = ref["case"], ref["weights"]
    for (emb, pos, _), (toks, logits) in zip(ref["prompts"], ref["runs"]):
        T, n = emb.shape[0], 8
        E = torch.from_numpy(weights["model.embed_tokens.weight"]).double()
        x = torch.cat([torch.from_numpy(emb).double(), E[torch.from_numpy(toks[:n - 1])]])
        nxt = int(pos.max()) + 1
        p_all = torch.cat([torch.from_numpy(pos).long(), (nxt + torch.arange(n - 1))[None, :].repeat(3, 1)], dim=1)
        full = _full_forward(case, weights, x, p_all)[T - 1:]
        err = float((full - logits[:n]).abs().max())
        print(f"case {name} T={T}: cached vs full {err:.3e}")
        assert err < 1e-10


def test_reference_equals_transformers_qwen2_vl_text_model():
    """An outside implementation where one is installed (never required): the Qwen2-VL text model on a tiny configuration, same weights, same position ids."""
    pytest.importorskip("transformers")
    try:
        from transformers.models.qwen2_vl.configuration_qwen2_vl import Qwen2VLTextConfig
        from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
        case = R.LmCase("Q", 64, 2, 4, 2, 16, 96, 97, (2, 3, 3), qkv_bias=True, tie=False)    # (its head_dim is hidden / heads and its q / k / v carry a bias)
        cfg = Qwen2VLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=case.eps,
                                rope_parameters={"rope_type": "default", "rope_theta": case.theta, "mrope_section": [2, 3, 3]}, max_position_embeddings=128,
                                attn_implementation="eager", bos_token_id=None, eos_token_id=None, pad_token_id=None)
        model = Qwen2VLTextModel(cfg).double().eval()
    except (ImportError, TypeError, ValueError, AttributeError) as e:
        pytest.skip(f"this transformers version builds the Qwen2-VL text model differently: {e}")
    weights = R.make_lm(case, 3)
    sd = {k[len("model."):]: torch.from_numpy(v).double() for k, v in weights.items() if k.startswith("model.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    emb, pos, _ = R.make_prompt(case, weights, 37, 3)
    with torch.no_grad():
        theirs = model(inputs_embeds=torch.from_numpy(emb).double()[None], position_ids=torch.from_numpy(pos).long()[:, None, :]).last_hidden_state[0]
    ours = R.RefLM(case, weights, torch.float64).forward_chunk(torch.from_numpy(emb).double(), torch.from_numpy(pos).long(), [None] * case.L)
    err = float((theirs - ours).abs().max())
    print(f"reference vs transformers Qwen2VLTextModel: {err:.3e}")
    # their rotary table is computed in f32 whatever the model's dtype: cos / sin of an f32 angle up to 36 rad carry up to 36 x 2^-24 = 2e-6 each, which two layers
    # pass on to hidden values of order 1; a structural difference (any fault of the list below) moves them by 1e-2 and more
    assert err < 1e-4


@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_fault_moves_the_logits_far_beyond_the_tolerance(fault):
    """A reference that could not tell these variants apart would pin nothing.  Every fault is shown on case A's 37-position prompt with the image block (grouping by 2,
    unequal sections), under teacher forcing with the sound model's tokens; the place of eps on case C, whose token rows are small enough for eps to matter."""
    ref = R.reference_for("C" if fault == "eps_outside_sqrt" else "A")
    case, weights, tol = ref["case"], ref["weights"], ref["tol"]
    emb, pos, _ = ref["prompts"][2]
    toks, logits = ref["runs"][2]
    _, bad = R.RefLM(case, weights, torch.float64, fault=fault).generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=R.TEACHER_STEPS, forced_tokens=toks)
    moved = float((bad - logits[:R.TEACHER_STEPS]).abs().max())
    print(f"fault {fault}: moves the logits by {moved:.3e} = {moved / tol:.0f} x tol ({tol:.3e})")
    assert moved > 100 * tol


@pytest.mark.parametrize("name", list(R.CASES))
def test_seeds_are_greedy_safe(name):
    """A condition on the inputs: at every generated step of every prompt the f64 margin between the best and the second-best logit exceeds 4 tol, so a model within
    tol of f64 picks the same token and the GPU test may demand exact token equality with no step left out."""
    ref = R.reference_for(name)
    for (emb, _, _), (toks, logits) in zip(ref["prompts"], ref["runs"]):
        m = R.greedy_margins(logits)
        print(f"case {name} T={emb.shape[0]}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} least margin {m.min():.3e} = {m.min() / ref['tol']:.1f} x tol")
        assert len(toks) == R.FREE_STEPS and m.min() > 4 * ref["tol"]
    assert ref["tol"] >= 2.0 ** -19 and ref["noise"] > 0
    # the eos test: the 6th token of the 17-position prompt must not occur among its first five
    toks = ref["runs"][1][0]
    if name == "A":
        assert toks[5] not in toks[:5]


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_long_cache_seeds_are_greedy_safe(name):
    """The same condition for the long-cache cases: both sequences (T positions and its one-position step mate), every one of the LONG_STEPS steps."""
    ref = R.long_reference_for(name)
    assert [p[0].shape[0] for p in ref["prompts"]] == [ref["T"], 1]
    for (emb, pos, _), (toks, logits) in zip(ref["prompts"], ref["runs"]):
        m = R.greedy_margins(logits)
        print(f"case {name} T={emb.shape[0]}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} least margin {m.min():.3e} = {m.min() / ref['tol']:.1f} x tol")
        assert len(toks) == R.LONG_STEPS and m.min() > 4 * ref["tol"]
    assert ref["tol"] >= 2.0 ** -19 and ref["noise"] > 0
    emb, pos, _ = ref["prompts"][0]
    T = ref["T"]
    pre = (T - 12) // 2
    assert 0 < pre and pre + 12 < T and len(set(pos[:, pre + 5].tolist())) > 1          # the image block sits in the middle


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_a_dropped_key_at_any_loop_boundary_moves_the_long_cache_logits(name):
    """A condition on the inputs: an attention loop that lost one key -- the last of a wave's first turn, the first of the next wave, of the next unrolled turn, of the next
    outer iteration, or the newest prompt key -- must be visible.  For every such key j the skip_key variant moves the teacher-forced f64 logits by more than 20 tol."""
    ref = R.long_reference_for(name)
    case, T, tol = ref["case"], ref["T"], ref["tol"]
    (kpw, turn, ut), js = R.attn_boundaries(case.head_dim, T)
    assert {kpw - 1, kpw, turn - 1, turn, T - 1} <= set(js) or turn >= T
    emb, pos, _ = ref["prompts"][0]
    toks, logits = ref["runs"][0]
    least = None
    for j in js:
        _, bad = R.RefLM(case, ref["weights"], torch.float64, skip_key=j).generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=R.LONG_STEPS, forced_tokens=toks)
        moved = float((bad - logits).abs().max())
        least = (moved, j) if least is None or moved < least[0] else least
        assert moved > 20 * tol, (name, j, moved / tol)
    print(f"case {name} head size {case.head_dim} T={T}: kpw {kpw} turn {turn} U x turn {ut}, keys {js}: least skip_key movement {least[0] / tol:.0f} x tol at j = {least[1]}")


def test_skip_key_changes_only_rows_beyond_the_key():
    ref = R.reference_for("A")
    emb, pos, _ = ref["prompts"][2]
    x, p3 = torch.from_numpy(emb).double(), torch.from_numpy(pos).long()
    good = R.RefLM(ref["case"], ref["weights"]).forward_chunk(x, p3, [None] * ref["case"].L)
    bad = R.RefLM(ref["case"], ref["weights"], skip_key=20).forward_chunk(x, p3, [None] * ref["case"].L)
    assert torch.equal(good[:21], bad[:21]) and all(float((good[t] - bad[t]).abs().max()) > 0 for t in range(21, 37))


def test_the_new_cases_take_the_kernel_paths_their_comments_name():
    """The arithmetic of lm_decode.hip's grids and loops, from its own header (compiled for the host), at the shapes of the cases."""
    cs = R.CASES
    V, W = cs["V"], cs["W"]
    g = R.kernel_geometry((V.vocab, 2 * W.F, W.D, 8192 // 2, 3080))
    per = g["waves"] * g["rows_per_wave"]
    # query heads per kv head: 1 / 2 run <1> / <2>, 3 .. 7 run <4>, 8 and more <8>, ceil(G / GT) chunks along gridDim.z
    G = {n: c.heads // c.kv_heads for n, c in cs.items()}
    assert (G["E"], G["F"], G["G"], G["H"]) == (8, 7, 3, 12) and g["max_gt"] == 8
    assert G["F"] % 4 == 3 and G["G"] < 4 and G["H"] % 8 == 4                 # a partial chunk of heads in F (the second), G (the only one) and H (the second of <8>)
    assert max(G[n] for n in "ABCD") == 2                                     # what the first four cases left out
    idle = lambda dh: 64 // g["kpw"][dh] - dh // 4                              # noqa: E731  lanes of a key's lane group beyond the head size
    assert idle(cs["G"].head_dim) == 3 and 64 // g["kpw"][20] == 8 and [idle(c.head_dim) for c in (cs["A"], cs["B"], cs["C"], cs["D"], cs["E"], cs["F"])] == [0] * 6
    assert idle(R.LONG_CASES["LB"][0].head_dim) == 12 and idle(R.LONG_CASES["LE"][0].head_dim) == 1 and idle(R.LONG_CASES["LC"][0].head_dim) == 3
    # rows kernels: one row group up to N = per x 512; the largest N of the first four cases (2 F of D) stays below
    assert g["rows"][8192 // 2] == (1, 512) and g["rows"][3080][0] == 1 and per == 8
    # V: the lm-head has 3 row groups per workgroup, 417 workgroups, so lm_combine's 256 threads stride over the partials; K = 32 is staged once
    assert g["rows"][V.vocab] == (3, 417) and 417 > g["threads"] and V.D <= g["kc"] and not V.tie
    # W: gate / up has 2 row groups and K = D = 1028 is two staging chunks (1024 + 4), restaged per group; the down projection's K = F = 2052 ends in 4 columns as well
    assert g["rows"][2 * W.F] == (2, 257)
    assert g["kc"] < W.D < 2 * g["kc"] and W.D % g["kc"] == 4 and W.F % g["kc"] == 4 and g["rows"][W.D][0] == 1
    # equal maxima: the five places of a pair
    d = R.tie_distances()
    assert [d[k] for k in R.TIE_PLACES] == [1, 2, 8, 24, 4992, 16, 48, 9984]
    # far: workgroup w and w + 208 hold a pair, which two different threads of lm_combine read; 9984 pairs the last workgroup (416) with the first
    assert d["far_workgroup"] % (3 * per) == 0 and 0 < (d["far_workgroup"] // (3 * per)) % g["threads"] and d["d9984"] == 416 * 3 * per < V.vocab


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_the_long_cases_cross_the_boundaries_of_the_key_loop(name):
    """Row r of a step attends n = p_r + 1 keys; the forced steps take n from T to T + LONG_STEPS - 1.  That range crosses a multiple of U x turn, or of turn where
    U x turn lies beyond what a test can pin; the one-position mate has n = 1 .. LONG_STEPS in the same steps."""
    case, T = R.LONG_CASES[name]
    (kpw, turn, ut), _ = R.attn_boundaries(case.head_dim, T)
    lo, hi = T, T + R.LONG_STEPS - 1
    b = ut if ut <= hi else turn
    assert any(lo <= m < hi for m in range(b, hi + 1, b)), (name, kpw, turn, ut, T)
    assert hi > turn                                                               # all eight waves hold keys
    if name in ("LA", "LB", "LC"):
        assert hi > 2 * ut                                                         # a second and a third outer iteration
    else:
        assert turn < hi <= ut and hi > (hi // turn) * turn                        # one outer iteration whose unroll is used in part: the `break`
    print(f"case {name}: head size {case.head_dim} kpw {kpw} turn {turn} U x turn {ut}; n = {lo} .. {hi} crosses {[m for m in range(b, hi + 1, b) if lo <= m < hi]}")


@pytest.mark.parametrize("place", R.TIE_PLACES)
def test_equal_maxima_models_keep_the_winning_pair_clear_of_the_rest(place):
    """A condition on the inputs of the equal-maxima GPU test: with lm-head rows paired d apart, the f64 margin between the winning pair and the best other row exceeds
    4 tol at every forced step, and the forced tokens are the lower row of their pair."""
    d = R.tie_distances()[place]
    ref = R.tie_reference_for(d)
    canon, w = ref["canon"], ref["weights"]["lm_head.weight"]
    assert np.array_equal(w, w[canon]) and (canon <= np.arange(len(canon))).all() and int((canon != np.arange(len(canon))).sum()) >= (len(canon) - d) // 2
    least = min(float(R.pair_margins(l64, canon).min()) for _, l64 in ref["runs"])
    print(f"equal maxima {place} d={d}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} least pair margin {least / ref['tol']:.1f} x tol")
    assert least > 4 * ref["tol"] and ref["tol"] >= 2.0 ** -19 and ref["noise"] > 0
    for t64, _ in ref["runs"]:
        assert np.array_equal(canon[t64], t64)
    if place != "d9984":      # (9984 pairs 23 rows only: its winners are single rows, and the test pins the pairs' logits)
        assert any((t64 + d < len(canon)).any() for t64, _ in ref["runs"])          # winners that do have a copy, d rows up


def test_an_eos_exists_that_ends_every_sequence_early():
    pick = R.all_end_choice(R.reference_for("A"))
    assert pick is not None
    i, j, eos, nj = pick
    ti, tj = R.reference_for("A")["runs"][i][0], R.reference_for("A")["runs"][j][0]
    assert ti[0] == eos and tj[nj - 1] == eos and eos not in tj[:nj - 1] and 1 < nj < R.FREE_STEPS


def test_position_ids_have_three_different_axes_and_end_below_T():
    for T in (17, 37):
        p = R.make_positions(T)
        assert p.shape == (3, T) and not np.array_equal(p[0], p[1]) and not np.array_equal(p[1], p[2]) and not np.array_equal(p[0], p[2])
        assert p.max() + 1 < T
    assert np.array_equal(R.make_positions(1), np.zeros((3, 1), np.int32))


def _write_safetensors(path, tensors):
    header, blobs, off = {}, [], 0
    for name, (a, dt) in tensors.items():
        b = np.ascontiguousarray(a).tobytes()
        header[name] = {"dtype": dt, "shape": list(a.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    h = json.dumps(header).encode()
    h += b" " * (-len(h) % 8)
    path.write_bytes(struct.pack("<Q", len(h)) + h + b"".join(blobs))


def test_safetensors_reader_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 7)).astype(np.float32)
    b = R.to_bf16_bits(rng.standard_normal((3, 4, 2)).astype(np.float32))
    c = rng.standard_normal(9).astype(np.float32)
    f = tmp_path / "m.safetensors"
    _write_safetensors(f, {"model.a": (a, "F32"), "model.b": (b, "BF16"), "other.c": (c, "F32")})
    got = vl.read_safetensors(f)
    assert set(got) == {"model.a", "model.b", "other.c"}
    assert got["model.a"].dtype == np.float32 and np.array_equal(got["model.a"], a)
    assert got["model.b"].dtype == np.uint16 and np.array_equal(got["model.b"], b) and np.array_equal(got["other.c"], c)
    assert set(vl.read_safetensors(f, names=lambda n: n.startswith("model."))) == {"model.a", "model.b"}
    assert np.array_equal(R.bf16_bits_to_f32(R.to_bf16_bits(R.bf16_bits_to_f32(b))), R.bf16_bits_to_f32(b))
    try:
        from safetensors import safe_open
    except ImportError:
        safe_open = None
    if safe_open is not None:
        with safe_open(str(f), framework="pt") as sf:
            assert np.array_equal(sf.get_tensor("model.a").numpy(), a)
            assert np.array_equal(sf.get_tensor("model.b").view(torch.int16).numpy().view(np.uint16), b)
    bad = tmp_path / "bad.safetensors"
    bad.write_bytes(struct.pack("<Q", 1 << 40) + b"{}")
    with pytest.raises(api.OCRError) as e:
        vl.read_safetensors(bad)
    assert e.value.code == api.OAR_MODEL_LOAD


def test_config_from_hf_json():
    d = {"hidden_size": 1024, "intermediate_size": 3072, "num_attention_heads": 16, "num_hidden_layers": 18, "num_key_value_heads": 2, "head_dim": 128, "vocab_size": 103424,
         "rms_norm_eps": 1e-5, "rope_theta": 500000.0, "image_token_id": 100295, "video_token_id": 101307, "vision_start_token_id": 101305, "vision_end_token_id": 101306,
         "hidden_act": "silu", "use_bias": False, "rope_scaling": {"mrope_section": [16, 24, 24], "rope_type": "default", "type": "default"}, "vision_config": {"hidden_size": 1152}}
    c = vl.CausalLMConfig.from_hf_json(d)
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size, c.vocab_size) == (1024, 18, 16, 2, 128, 3072, 103424)
    assert c.mrope_section == [16, 24, 24] and c.rope_theta == 500000.0 and c.rms_norm_eps == 1e-5 and not c.qkv_bias and not c.tie_word_embeddings
    assert c.num_attention_heads * c.head_dim != c.hidden_size          # ERNIE-4.5-0.3B: 16 x 128 = 2048 over a width of 1024
    q = vl.CausalLMConfig.from_hf_json({"hidden_size": 64, "intermediate_size": 96, "num_attention_heads": 4, "num_hidden_layers": 2, "vocab_size": 50, "tie_word_embeddings": True,
                                        "attention_bias": True}, max_positions=128)
    assert q.head_dim == 16 and q.num_key_value_heads == 4 and q.mrope_section == [8, 0, 0] and q.qkv_bias and q.tie_word_embeddings and q.max_positions == 128
    cc = c.to_c()
    assert list(cc.mrope_section) == [16, 24, 24] and cc.kv_heads == 2 and cc.max_sequences == 16


def _cfg_of(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, num_key_value_heads=case.kv_heads, head_dim=case.head_dim, intermediate_size=case.F,
             vocab_size=case.vocab, rms_norm_eps=case.eps, rope_theta=case.theta, mrope_section=list(case.mrope_section), qkv_bias=case.qkv_bias, tie_word_embeddings=case.tie,
             max_positions=64, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d)


def test_create_checks_its_arguments_before_it_touches_a_device():
    build.build_lib()
    case = R.CASES["A"]
    weights = R.make_lm(case, 0)
    rejected = [(dict(head_dim=132, mrope_section=[22, 22, 22]), api.OAR_UNSUPPORTED_OP), (dict(head_dim=6, mrope_section=[1, 1, 1]), api.OAR_UNSUPPORTED_OP),
                (dict(mrope_section=[2, 3, 2]), api.OAR_INVALID_INPUT), (dict(num_key_value_heads=3), api.OAR_INVALID_INPUT), (dict(max_sequences=17), api.OAR_INVALID_INPUT),
                (dict(max_sequences=0), api.OAR_INVALID_INPUT)]
    for kw, code in rejected:
        with pytest.raises(api.OCRError) as e:
            vl.CausalLM.from_state_dict(_cfg_of(case, **kw), weights)
        assert e.value.code == code, (kw, str(e.value))
    short = {k: v for k, v in weights.items() if k != "model.layers.1.mlp.up_proj.weight"}
    with pytest.raises(api.OCRError) as e:
        vl.CausalLM.from_state_dict(_cfg_of(case), short)
    assert e.value.code == api.OAR_INVALID_INPUT and "model.layers.1.mlp.up_proj.weight" in str(e.value)
    wrong = dict(weights)
    wrong["model.layers.0.self_attn.k_proj.weight"] = weights["model.layers.0.self_attn.q_proj.weight"]
    with pytest.raises(api.OCRError) as e:
        vl.CausalLM.from_state_dict(_cfg_of(case), wrong)
    assert e.value.code == api.OAR_INVALID_INPUT and "wrong shape" in str(e.value)
    mixed = dict(weights)
    mixed["model.layers.0.mlp.down_proj.weight"] = R.to_bf16_bits(weights["model.layers.0.mlp.down_proj.weight"])
    with pytest.raises(api.OCRError) as e:
        vl.CausalLM.from_state_dict(_cfg_of(case), mixed)
    assert e.value.code == api.OAR_INVALID_INPUT
    if api.device_count() == 0:      # a sound table passes every check and fails loudly at the device: no CPU fallback
        with pytest.raises(api.OCRError) as e:
            vl.CausalLM.from_state_dict(_cfg_of(case), weights)
        assert e.value.code == api.OAR_DEVICE
