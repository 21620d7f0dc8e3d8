"""The front of a vision transformer on the frozen int8 plan (fuse_inference(patch_embed=True)), on the host: the dry-run decisions for
the small ViT, the spellings that are taken and those left alone (with the report's reason), the plan without the flag, and the argument
checks of dlmcq_patch_rows_f32 / dlmcq_tokens_assemble_f32 that need no GPU (wrappers marked calibrated by hand, as in
test_transformer_host.py)."""
import ctypes
import operator
import os
import re

import pytest
import torch
from torch import nn

import transformer_nets as T
import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import PatchRowsLayer, TokenAssembleLayer, fuse_inference
from plan_dump import plan_text
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = (N.FORM_ZEROPOINT, 0, 255, 1.0, 0.0, False)      # every wrapper's input quantiser as `fsptq` leaves it


def nodes(gm, prefix):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith(prefix)]


def targets(users):
    return sorted(str(u.target) for u in users)


class Front(nn.Module):
    """The front of a ViT with the pieces the pass looks at open to the test: 32^2 images, 8^2 patches, 3 channels, width 64 - the
    small ViT's numbers.  `rearrange(self, img)` and `assemble(self, x)` are the two spellings; `pos_rows` the position embedding's length."""

    def __init__(self, rearrange=None, assemble=None, in_features=192, pos_rows=17, patch=8, image=32):
        super().__init__()
        self.p, self.g = patch, image // patch
        self.embed = nn.Linear(in_features, 64)
        self.other = nn.Linear(in_features, 64)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, 64))
        self.pos_embedding = nn.Parameter(torch.zeros(1, pos_rows, 64))
        self.fc = nn.Linear(64, 64)
        self.rearrange = rearrange or Front.rows
        self.assemble = assemble or Front.cat_add

    def rows(self, img):
        p, g = self.p, self.g
        return img.reshape(-1, 3, g, p, g, p).permute(0, 2, 4, 3, 5, 1).reshape(-1, g * g, p * p * 3)

    def cat_add(self, x):
        return torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1) + self.pos_embedding

    def forward(self, img):
        return self.fc(self.assemble(self, self.embed(self.rearrange(self, img))))


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True), fuse_inference(fsptq(make()), dry_run=True, patch_embed=True, **kw)


# ------------------------------------------------------------------------------------------- the small ViT
@pytest.mark.parametrize("make", [T.small_vit, lambda: W.ViT(32, 8, 10, dim=64, depth=2, heads=2, mlp_dim=128, dim_head=32)],
                         ids=["transformer_nets", "workloads"])
def test_small_vit_decisions(make):
    off, on = both(make)
    ro, rn = off.fusion_report, on.fusion_report
    assert (rn.patch_rows, rn.token_assemblies, rn.patch_embed_left) == (1, 1, [])
    assert (ro.patch_rows, ro.token_assemblies, ro.patch_embed_left) == (0, 0, [])
    assert "patch rows on the plan=1" in repr(rn) and "token assemblies on the plan=1" in repr(rn)
    assert "patch rows" not in repr(ro) and "token assemblies" not in repr(ro)
    mods = dict(on.named_modules())
    (pr,), (tk,) = nodes(on, "_int8_patch_rows_"), nodes(on, "_int8_tokens_")
    assert not any(isinstance(m, (PatchRowsLayer, TokenAssembleLayer)) for m in off.modules())
    # the patch rows: read the image, hand the embedding (the first plan node) their codes, nobody reads the fp32 rows
    m = mods[pr.target]
    assert isinstance(m, PatchRowsLayer) and pr.args[0].op == "placeholder"
    gets = {u.args[1]: u for u in pr.users}
    assert sorted(gets) == [1] or not gets[0].users
    assert targets(gets[1].users) == ["_int8_plan_0"]
    assert (m.want_out, m.c, m.c_pad, m.pad_code, m.emit_shift, m.emit.key) == (False, 192, 192, 0, False, KEY)
    assert (m.channels, m.grid, m.patch, m.tokens) == (3, (4, 4), 8, 16)
    d = m.decision
    assert (d.c, d.g1, d.g2, d.p, d.want_out, d.takers) == (3, 4, 4, 8, False, ("_int8_plan_0",)) and len(d.chain) == 3
    # the token tensor: the embedding's fp32 output and the two parameters in, one tensor out
    t = mods[tk.target]
    assert isinstance(t, TokenAssembleLayer) and (t.rows, t.c) == (None, 64)
    x, cls, pos = tk.args
    assert x.target is operator.getitem and x.args == (next(n for n in on.graph.nodes if n.target == "_int8_plan_0"), 0)
    assert (cls.op, cls.target, pos.op, pos.target) == ("get_attr", "cls_token", "get_attr", "pos_embedding")
    assert len(t.decision.chain) == 3 and t.decision.cls == cls.name
    # what is left of the replaced ops: nothing
    assert not [n for n in on.graph.nodes if n.target in (torch.cat, "expand") or (n.target == "permute" and len(n.args) == 7)]
    assert [n for n in off.graph.nodes if n.target in (torch.cat, "expand") or (n.target == "permute" and len(n.args) == 7)]
    assert len(list(on.graph.nodes)) < len(list(off.graph.nodes))
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem", "layer_norms", "gelus"):
        assert getattr(rn, f) == getattr(ro, f), f      # whatever the main pass decided stays
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 32))                    # a dry-run stand-in cannot be run
    with pytest.raises(RuntimeError):
        t(torch.zeros(1, 16, 64), torch.zeros(1, 1, 64), torch.zeros(1, 17, 64))


def test_with_every_transformer_flag():
    on = fuse_inference(fsptq(T.small_vit()), dry_run=True, patch_embed=True, layer_norms=True, gelu=True, attention=True)
    r = on.fusion_report
    assert (r.patch_rows, r.token_assemblies, r.layer_norms, r.gelus, r.attentions) == (1, 1, 5, 2, 2)
    (tk,) = nodes(on, "_int8_tokens_")
    # the token tensor is read by block 0's LayerNorm node and by its shortcut add
    assert any(str(u.target).startswith("_int8_layernorm_") for u in tk.users) and len(tk.users) == 2


def test_vit_small_16():
    on = fuse_inference(fsptq(W.vit_small()), dry_run=True, patch_embed=True)
    (pr,) = nodes(on, "_int8_patch_rows_")
    m = dict(on.named_modules())[pr.target]
    assert (m.channels, m.grid, m.patch, m.tokens, m.c, m.want_out) == (3, (14, 14), 16, 196, 768, False)
    assert on.fusion_report.token_assemblies == 1


# ------------------------------------------------------------------------------------------- spellings: taken
def _view(self, img):
    return img.view(-1, 3, 4, 8, 4, 8).permute((0, 2, 4, 3, 5, 1)).reshape((-1, 16, 192))


TAKEN = {
    "pos_first": lambda self, x: self.pos_embedding + torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1),
    "torch_add": lambda self, x: torch.add(torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), 1), self.pos_embedding),
    "static_batch": lambda self, x: torch.cat((self.cls_token.expand(2, -1, -1), x), dim=1) + self.pos_embedding,
}


def _iadd(self, x):
    x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
    x += self.pos_embedding
    return x


def _sliced(self, x):
    x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
    x += self.pos_embedding[:, :17]
    return x


TAKEN["iadd"] = _iadd


@pytest.mark.parametrize("name", sorted(TAKEN))
def test_token_spellings_taken(name):
    off, on = both(lambda: Front(assemble=TAKEN[name]))
    r = on.fusion_report
    assert (r.patch_rows, r.token_assemblies, r.patch_embed_left) == (1, 1, []), r
    assert not [n for n in on.graph.nodes if n.target in (torch.cat, "expand")]


def test_the_static_slice_of_a_longer_position_embedding_is_taken():
    off, on = both(lambda: Front(assemble=_sliced, pos_rows=50))
    assert (on.fusion_report.token_assemblies, on.fusion_report.patch_embed_left) == (1, [])
    (tk,) = nodes(on, "_int8_tokens_")
    assert dict(on.named_modules())[tk.target].rows == 17 and tk.args[2].op == "get_attr" and len(dict(on.named_modules())[tk.target].decision.chain) == 4
    assert not [n for n in on.graph.nodes if n.target in (torch.cat, "expand")]


def test_view_and_tuple_spellings_of_the_rearrangement_are_taken():
    off, on = both(lambda: Front(rearrange=_view))
    assert (on.fusion_report.patch_rows, on.fusion_report.patch_embed_left) == (1, [])


def test_a_second_fp32_reader_gets_the_fp32_rows():
    class Two(Front):
        def forward(self, img):
            r = self.rearrange(self, img)
            return self.fc(self.assemble(self, self.embed(r) + self.other(r))) + r.sum()
    off, on = both(Two)
    (pr,) = nodes(on, "_int8_patch_rows_")
    m = dict(on.named_modules())[pr.target]
    gets = {u.args[1]: u for u in pr.users}
    assert m.want_out and len(gets[1].users) >= 1 and len(gets[0].users) == 1 and len(m.decision.takers) >= 1


# ------------------------------------------------------------------------------------------- left alone
def _other_permute(self, img):
    return img.reshape(-1, 3, 4, 8, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(-1, 16, 192)


def _second_reader(self, img):
    t = img.reshape(-1, 3, 4, 8, 4, 8).permute(0, 2, 4, 3, 5, 1)
    return t.reshape(-1, 16, 192) + t.sum()


def _p6(self, img):       # 12^2 images of 16 channels in 6^2 patches: 4 tokens of 576 features (a Linear the plan takes), but 6 % 4 != 0
    return img.reshape(-1, 16, 2, 6, 2, 6).permute(0, 2, 4, 3, 5, 1).reshape(-1, 4, 576)


LEFT = {
    "another_permute": (lambda: Front(rearrange=_other_permute), "a permute", 1),
    "a_second_reader_of_the_permuted_tensor": (lambda: Front(rearrange=_second_reader), "second reader", 1),
    "in_features_differ": (lambda: Front(in_features=256), "in-features", 1),
    "p_mod_4": (lambda: Front(rearrange=_p6, in_features=576, pos_rows=5), "no multiple of 4", 1),
    "pos_of_the_wrong_length": (lambda: Front(pos_rows=18), "position embedding of 18 rows for 16 + 1 tokens", 0),
    "pos_slice_of_the_wrong_length": (lambda: Front(assemble=lambda self, x: torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
                                                    + self.pos_embedding[:, :16], pos_rows=18), "position embedding of 16 rows", 0),
    "cat_along_another_dim": (lambda: Front(assemble=lambda self, x: torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=2)
                                            + self.pos_embedding), "dim 1", 0),
}


@pytest.mark.parametrize("name", sorted(LEFT))
def test_left_alone(name):
    make, why, tokens_taken = LEFT[name]
    ref = fuse_inference(fsptq(make()), dry_run=True)
    on = fuse_inference(fsptq(make()), dry_run=True, patch_embed=True)
    r = on.fusion_report
    kept = lambda gm: [n.target for n in gm.graph.nodes if n.target in (torch.cat, "expand", "permute")]  # noqa: E731
    if tokens_taken:      # the rearrangement is left alone (the token tensor behind it is taken on its own)
        assert (r.patch_rows, r.token_assemblies) == (0, 1) and not nodes(on, "_int8_patch_rows_")
        assert kept(on) == ["permute"] and kept(ref) == ["permute", "expand", torch.cat]
    else:
        assert (r.patch_rows, r.token_assemblies) == (1, 0) and not nodes(on, "_int8_tokens_")
        assert kept(on) == ["expand", torch.cat] and kept(ref) == ["permute", "expand", torch.cat]
    assert len(r.patch_embed_left) == 1 and why in r.patch_embed_left[0][1], r.patch_embed_left
    assert "patch embedding left alone" in repr(r)


@pytest.mark.parametrize("name", ["another_permute", "a_second_reader_of_the_permuted_tensor", "in_features_differ", "p_mod_4"])
def test_a_refused_rearrangement_leaves_the_graph_as_it_was(name):
    """... node for node, where the token tensor behind it is not there to be taken either."""
    make = LEFT[name][0]

    def plain(self, x):
        return x
    a = make()
    b = make()
    a.assemble = b.assemble = plain
    ref = fuse_inference(fsptq(a), dry_run=True)
    on = fuse_inference(fsptq(b), dry_run=True, patch_embed=True)
    assert str(on.graph) == str(ref.graph) and (on.fusion_report.patch_rows, on.fusion_report.token_assemblies) == (0, 0)
    assert len(on.fusion_report.patch_embed_left) == 1


@pytest.mark.parametrize("name", ["pos_of_the_wrong_length", "pos_slice_of_the_wrong_length", "cat_along_another_dim"])
def test_a_refused_token_tensor_leaves_the_graph_as_it_was(name):
    make = LEFT[name][0]
    a, b = make(), make()
    a.rearrange = b.rearrange = lambda self, img: img.reshape(-1, 16, 192)      # (rows given as they are: nothing for the first half of the pass)
    ref = fuse_inference(fsptq(a), dry_run=True)
    on = fuse_inference(fsptq(b), dry_run=True, patch_embed=True)
    assert str(on.graph) == str(ref.graph) and (on.fusion_report.patch_rows, on.fusion_report.token_assemblies) == (0, 0)


# ------------------------------------------------------------------------------------------- the flag off
@pytest.mark.parametrize("make", [T.small_vit, W.mobilenet_v2, W.resnet50], ids=["small_vit", "mobilenet_v2", "resnet50"])
def test_flag_off_is_the_plan_as_it_was(make):
    plain = fuse_inference(fsptq(make()), dry_run=True)
    explicit = fuse_inference(fsptq(make()), dry_run=True, patch_embed=False)
    assert plan_text(plain) == plan_text(explicit) and str(plain.graph) == str(explicit.graph)
    assert not nodes(plain, "_int8_patch_rows_") and not nodes(plain, "_int8_tokens_")
    assert "patch rows" not in plan_text(plain) and "token assemblies" not in plan_text(plain)


@pytest.mark.parametrize("make", [W.mobilenet_v2, W.resnet50], ids=["mobilenet_v2", "resnet50"])
def test_flag_on_changes_nothing_where_there_is_nothing_to_take(make):
    off, on = both(make)
    assert plan_text(off) == plan_text(on) and on.fusion_report.patch_embed_left == []


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
@pytest.mark.parametrize("name, count", [("dlmcq_patch_rows_f32", 18), ("dlmcq_tokens_assemble_f32", 11)])
def test_header_exports_and_ctypes_table_agree(name, count):
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint " + name + r"\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES[name]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == count
    fn = getattr(N.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    if name == "dlmcq_patch_rows_f32":      # exactly the quantiser arguments of dlmcq_gelu_nhwc_f32 (and the stream)
        assert list(args[-7:]) == list(N.SIGNATURES["dlmcq_gelu_nhwc_f32"][1][-7:])


# ------------------------------------------------------------------------------------------- the entry points, without a GPU
def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _rows(img=1 << 12, out=1 << 13, codes=1 << 14, b=2, c=3, gh=4, gw=4, p=8, sb=3072, sc=1024, sh=32, scale=1 << 15, zp=None, lo=0,
          hi=255, form=None, g=0.0):
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_patch_rows_f32(_p(img), _p(out), _p(codes), b, c, gh, gw, p, sb, sc, sh, _p(scale), _p(zp), lo, hi, form, g, None)


def _tok(e=1 << 12, cls=1 << 16, pos=1 << 17, out=1 << 13, b=2, t=16, c=64, es=64, osb=17 * 64, ost=64):
    return N.lib.dlmcq_tokens_assemble_f32(_p(e), _p(cls), _p(pos), _p(out), b, t, c, es, osb, ost, None)


EINVAL, ERANGE, EALIGN = -1, -2, -4
CONTROL_BITS = {"force_tiled": N.FORCE_TILED, "route_only": N.ROUTE_ONLY, "pipelined": N.PIPELINED, "chunk_major_in": N.FP32_IN_CHUNK_MAJOR,
                "chunk_major_out": N.FP32_OUT_CHUNK_MAJOR}
ROWS_REFUSED = {
    "negative_b": (dict(b=-1), EINVAL), "c_0": (dict(c=0), EINVAL), "gh_0": (dict(gh=0), EINVAL), "gw_0": (dict(gw=0), EINVAL),
    "p_0": (dict(p=0), EINVAL), "p_mod_4": (dict(p=6), EINVAL), "p_2": (dict(p=2), EINVAL),
    "sb_mod_4": (dict(sb=3074), EINVAL), "sc_mod_4": (dict(sc=1026), EINVAL), "sh_mod_4": (dict(sh=33), EINVAL), "sh_negative": (dict(sh=-32), EINVAL),
    "strip_past_the_lds": (dict(gw=86, p=16), EINVAL), "strip_just_past_the_lds": (dict(c=1, gw=1025, p=8), EINVAL), "p_past_256": (dict(p=260), EINVAL),
    "c_2_31": (dict(c=1 << 31), EINVAL), "gw_2_40": (dict(gw=1 << 40), EINVAL),
    "no_output": (dict(out=None, codes=None), EINVAL), "null_img": (dict(img=None), EINVAL), "codes_without_scale": (dict(scale=None), EINVAL),
    "lo_above_hi": (dict(lo=5, hi=4), EINVAL), "unknown_form": (dict(form=9), EINVAL), "range_wider_than_a_byte": (dict(lo=-128, hi=255), EINVAL),
    "shifted_emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), EINVAL),
    "img_misaligned": (dict(img=(1 << 12) + 4), EALIGN), "out_misaligned": (dict(out=(1 << 13) + 8), EALIGN),
    "codes_misaligned": (dict(codes=(1 << 14) + 4), EALIGN),
    "b_2_31": (dict(b=1 << 31), ERANGE), "strips_reach_2_31": (dict(b=1 << 16, gh=1 << 15), ERANGE),
    "rows_reach_2_31": (dict(b=1 << 16, gh=1 << 14, gw=2), ERANGE), "gh_2_31": (dict(b=1, gh=1 << 31), ERANGE),
    "image_lines_reach_2_31": (dict(b=1, gh=1 << 28), ERANGE),
    # two faults: the earlier check of map_codes_call's order answers
    "geometry_before_quantiser": (dict(p=6, scale=None), EINVAL), "quantiser_before_alignment": (dict(lo=5, hi=4, img=(1 << 12) + 4), EINVAL),
    "null_before_alignment": (dict(img=None, out=(1 << 13) + 8), EINVAL), "alignment_before_range": (dict(b=1 << 31, out=(1 << 13) + 8), EALIGN),
    **{k: (dict(form=N.FORM_ZEROPOINT | v), EINVAL) for k, v in CONTROL_BITS.items()},
}
TOKENS_REFUSED = {
    "negative_b": (dict(b=-1), EINVAL), "t_0": (dict(t=0), EINVAL), "c_0": (dict(c=0), EINVAL), "c_mod_4": (dict(c=66, es=68, ost=68), EINVAL),
    "e_stride_below_c": (dict(es=60), EINVAL), "e_stride_mod_4": (dict(es=66), EINVAL), "o_st_below_c": (dict(ost=60), EINVAL),
    "o_st_mod_4": (dict(ost=66, osb=17 * 66), EINVAL), "o_sb_mod_4": (dict(osb=17 * 64 + 2), EINVAL), "images_overlap": (dict(osb=16 * 64), EINVAL),
    "null_e": (dict(e=None), EINVAL), "null_cls": (dict(cls=None), EINVAL), "null_pos": (dict(pos=None), EINVAL), "null_out": (dict(out=None), EINVAL),
    "e_misaligned": (dict(e=(1 << 12) + 4), EALIGN), "cls_misaligned": (dict(cls=(1 << 16) + 8), EALIGN),
    "pos_misaligned": (dict(pos=(1 << 17) + 4), EALIGN), "out_misaligned": (dict(out=(1 << 13) + 8), EALIGN),
    "b_2_31": (dict(b=1 << 31), ERANGE), "rows_reach_2_31": (dict(b=1 << 27), ERANGE), "quads_reach_2_31": (dict(b=1 << 23), ERANGE),
    "null_before_alignment": (dict(e=None, out=(1 << 13) + 8), EINVAL), "alignment_before_range": (dict(b=1 << 31, out=(1 << 13) + 8), EALIGN),
}


@pytest.mark.parametrize("name", sorted(ROWS_REFUSED))
def test_patch_rows_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = ROWS_REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _rows(**kw) == rc


@pytest.mark.parametrize("name", sorted(TOKENS_REFUSED))
def test_tokens_refusals_need_no_gpu(name):
    kw, rc = TOKENS_REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _tok(**kw) == rc


def test_empty_problems_are_ok():
    assert _rows(b=0) == 0 and _rows(b=0, img=None, out=None, codes=None) == 0
    assert _tok(b=0) == 0 and _tok(b=0, e=None, cls=None, pos=None, out=None) == 0
