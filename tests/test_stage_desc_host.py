"""Host contract of the four stage-level C entries (lav_swin_block_fwd / _bwd, lav_bert_layer_fwd / _bwd): the descriptors the engine builds,
read back BY FIELD NAME through the ctypes declarations.  CPU tensors only (addresses, shapes and strides are all that is read); the C entries
themselves are replaced by a recorder, so nothing is launched and no device is needed."""
import ctypes as C
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

from lavender_amd import _lib as L, engine as E, hip as K

bf16, f32 = torch.bfloat16, torch.float32


def _param(*shape, t_ld=None):
    """a parameter as the arena leaves it: fp32 master (the tensor itself), bf16 copy, gradient view and -- for matrices -- the transposed copy"""
    p = torch.zeros(shape, dtype=f32)
    p._lav16, p._lavg = torch.zeros(shape, dtype=bf16), torch.zeros(shape, dtype=f32)
    if len(shape) == 2:
        p._lav16t = torch.zeros((shape[1], t_ld or shape[0] + 8), dtype=bf16)[:, :shape[0]]
    return p


def _linear(out_f, in_f):
    return NS(weight=_param(out_f, in_f), bias=_param(out_f))


def _norm(n):
    return NS(weight=_param(n), bias=_param(n), eps=1e-12)


class _Arena:
    """fused q | k | v views the way ParamArena.fused_view hands them out: (bf16 copy, gradient, fp32 master)"""

    def __init__(self, Hd):
        self.w = tuple(torch.zeros((3 * Hd, Hd), dtype=dt) for dt in (bf16, f32, f32))
        self.b = tuple(torch.zeros(3 * Hd, dtype=dt) for dt in (bf16, f32, f32))

    def fused_view(self, first, rows_total):
        return self.w if first.dim() == 2 else self.b


def _layer(Hd=64, ffn=128, heads=1):
    arena = _Arena(Hd)
    q = NS(weight=_param(Hd, Hd), bias=_param(Hd))
    q.weight._lav16t = torch.zeros((Hd, 3 * Hd + 64), dtype=bf16)[:, :3 * Hd]
    layer = NS(num_heads=heads, attention=NS(self=NS(query=q), output=NS(dense=_linear(Hd, Hd), LayerNorm=_norm(Hd))),
               intermediate=NS(dense=_linear(ffn, Hd)), output=NS(dense=_linear(Hd, ffn), LayerNorm=_norm(Hd)))
    layer.output.LayerNorm.eps = 1e-11                                      # distinct from the first LayerNorm's: ln_eps / ln2_eps must not swap
    layer._arena = lambda: layer.arena
    layer.arena = arena
    return layer


def _block(Cn=32, heads=1):
    attn = NS(qkv=_linear(3 * Cn, Cn), proj=_linear(Cn, Cn), relative_position_bias_table=_param(15, heads))
    return NS(num_heads=heads, keep_prob=0.8, attn=attn, mlp=NS(fc1=_linear(4 * Cn, Cn), fc2=_linear(Cn, 4 * Cn)), norm1=_norm(Cn), norm2=_norm(Cn))


class _Ctx:
    """what the stage functions use of an autograd context; `move()` re-homes the saved tensors, as a saved-tensor hook may"""

    def save_for_backward(self, *t):
        self.saved_tensors = t

    def mark_non_differentiable(self, *t):
        pass

    def move(self):
        self.saved_tensors = tuple(t.clone() for t in self.saved_tensors)


@pytest.fixture
def calls(monkeypatch):
    """the descriptor values handed to each of the four entries, instead of a launch"""
    got = {}
    for name in ("swin_block_fwd", "bert_layer_fwd"):
        monkeypatch.setattr(K, name, lambda fields, name=name: got.__setitem__(name, fields))
    for name in ("swin_block_bwd", "bert_layer_bwd"):
        monkeypatch.setattr(K, name, lambda fields, side, name=name: got.__setitem__(name, fields))
    monkeypatch.setattr(K, "ensure_stage_workspaces", lambda *a: None)
    monkeypatch.setattr(E, "_DW_SIDE", False)
    monkeypatch.setattr(E, "STREAM_DT", torch.float16)
    return got


def _read(layout, fields):
    """pack `fields` the way the entry does and read the descriptor back through its ctypes declaration: {field name: value}"""
    raw = C.create_string_buffer(C.sizeof(layout.struct))
    layout.pack.pack_into(raw, 0, *fields)
    obj = C.cast(raw, C.POINTER(layout.struct)).contents

    def walk(o):
        out = {}
        for name, ct in o._fields_:
            v = getattr(o, name)
            out.update(walk(v) if isinstance(v, C.Structure) else {name: v or 0})
        return out
    got = walk(obj)
    assert tuple(got) == layout.names
    return got


def _check(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for name, v in want.items():
        assert got[name] == pytest.approx(v, rel=1e-6) if isinstance(v, float) else got[name] == v, (name, got[name], v)


def _ptrs(**named):
    return {k: (0 if t is None else t.data_ptr()) for k, t in named.items()}


# ---- fusion layer --------------------------------------------------------------------------------------------------------------------------------
def _layer_param_fields(layer):
    a = layer.arena
    ao, inter, outp = layer.attention.output, layer.intermediate, layer.output
    return _ptrs(w_qkv=a.w[0], b_qkv=a.b[2], w_ao=ao.dense.weight._lav16, b_ao=ao.dense.bias, ln1_gamma=ao.LayerNorm.weight, ln1_beta=ao.LayerNorm.bias,
                 w_ff1=inter.dense.weight._lav16, b_ff1=inter.dense.bias, w_ff2=outp.dense.weight._lav16, b_ff2=outp.dense.bias,
                 ln2_gamma=outp.LayerNorm.weight, ln2_beta=outp.LayerNorm.bias)


def _layer_bwd_fields(layer):
    a = layer.arena
    q, ao, inter, outp = layer.attention.self.query, layer.attention.output, layer.intermediate, layer.output
    wt = dict(qkv=q.weight._lav16t, ao=ao.dense.weight._lav16t, ff1=inter.dense.weight._lav16t, ff2=outp.dense.weight._lav16t)
    want = {f"wt_{k}": t.data_ptr() for k, t in wt.items()}
    want.update({f"ldt_{k}": t.stride(0) for k, t in wt.items()})
    want.update(_ptrs(g_w_qkv=a.w[1], g_b_qkv=a.b[1], g_w_ao=ao.dense.weight._lavg, g_b_ao=ao.dense.bias._lavg, g_ln1_gamma=ao.LayerNorm.weight._lavg,
                      g_ln1_beta=ao.LayerNorm.bias._lavg, g_w_ff1=inter.dense.weight._lavg, g_b_ff1=inter.dense.bias._lavg,
                      g_w_ff2=outp.dense.weight._lavg, g_b_ff2=outp.dense.bias._lavg, g_ln2_gamma=outp.LayerNorm.weight._lavg,
                      g_ln2_beta=outp.LayerNorm.bias._lavg))
    return want


@pytest.mark.parametrize("resln,masked", list(itertools.product((False, True), (False, True))))
def test_fusion_layer_descriptors_hold_every_tensor_in_its_named_field(calls, resln, masked):
    n, Lq, Hd, ffn = 2, 5, 64, 128
    R = n * Lq
    layer = _layer(Hd, ffn)
    x = torch.zeros((R, Hd), dtype=bf16)
    key_mask = torch.ones((n, Lq), dtype=torch.int32) if masked else None
    carrier = (torch.zeros((R, Hd), dtype=torch.float16), torch.zeros(R), torch.zeros(R), torch.zeros(Hd), torch.zeros(Hd)) if resln else None
    ctx = _Ctx()
    y, pre2, mean2, rstd2 = E.BertLayerFn._forward_c(ctx, x, carrier, layer, E._layer_consts(layer), key_mask, n, Lq, 0.1, 0.2, True, 3, True)
    s1, s2 = ctx.seeds
    xs, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2s, st2 = ctx.saved_tensors[:11]
    assert pre2s is pre2 and mean2.data_ptr() == st2[0].data_ptr() and rstd2.data_ptr() == st2[1].data_ptr()

    def forward_fields(t, km, car):
        xs, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2 = t
        want = dict(n_seq=n, L=Lq, hidden=Hd, heads=1, ffn=ffn, p_hidden=0.1, p_attn=0.2, ln_eps=1e-12, ln2_eps=1e-11, seed1=s1, seed2=s2,
                    causal_from=3, stream_f16=1, y=y.data_ptr())
        want.update(_layer_param_fields(layer))
        want.update(_ptrs(key_mask=km, x=xs, qkv=qkv, cx=cx, lse=lse, pre1=pre1, mean1=st1[0], rstd1=st1[1], x1=x1, h_pre=h_pre, h=h, pre2=pre2,
                          mean2=st2[0], rstd2=st2[1]))
        want.update(_ptrs(**dict(zip(("res_pre", "res_mean", "res_rstd", "res_gamma", "res_beta"), car or (None,) * 5))))
        return want

    fwd = _read(K.BL_FWD, calls["bert_layer_fwd"])
    want = forward_fields(ctx.saved_tensors[:11], key_mask, carrier)
    want["seed_attn"] = fwd["seed_attn"]                                    # drawn inside the forward, in front of seed1 and seed2
    assert len({fwd["seed_attn"], s1, s2}) == 3
    _check(fwd, want)
    assert (fwd["key_mask"] == 0) == (not masked) and (fwd["res_pre"] == 0) == (not resln)      # NULL fields
    assert st1.shape == (2, R) and fwd["rstd1"] - fwd["mean1"] == 4 * R and fwd["rstd2"] - fwd["mean2"] == 4 * R

    for moved in (False, True):
        if moved:
            ctx.move()
        dy = torch.zeros((R, Hd), dtype=bf16)
        E.BertLayerFn._backward_c(ctx, dy)
        bwd = _read(K.BL_BWD, calls["bert_layer_bwd"])
        saved = ctx.saved_tensors
        if moved:
            car = tuple(saved[12:15]) + carrier[3:] if resln else None        # gamma / beta are parameters: they do not move
            want_f = dict(forward_fields(saved[:11], saved[11] if masked else None, car), seed_attn=fwd["seed_attn"])
            assert want_f["x"] != fwd["x"] and want_f["mean1"] != fwd["mean1"]
        else:
            want_f = fwd                                                    # same tensors: the forward section IS the forward descriptor
        _check({k: bwd[k] for k in K.BL_FWD.names}, want_f)
        rest = {k: v for k, v in bwd.items() if k not in K.BL_FWD.pos}
        want_b = _layer_bwd_fields(layer)
        want_b.update(dy=dy.data_ptr(), assign_mask=0, group_splits=K.group_splits_for(((Hd, ffn), (ffn, Hd), (Hd, Hd), (3 * Hd, Hd)), R),
                      splits_qkv=K.splits_for(3 * Hd, Hd, R), splits_ao=K.splits_for(Hd, Hd, R), splits_ff1=K.splits_for(ffn, Hd, R),
                      splits_ff2=K.splits_for(Hd, ffn, R))
        grads = ("d_pre2", "d_dense2", "dh", "d_x1", "d_pre1", "d_dense1", "d_cx", "dqkv", "dx")
        assert all(rest[g] for g in grads) and len({rest[g] for g in grads}) == len(grads)      # nine distinct fresh buffers
        _check({k: v for k, v in rest.items() if k not in grads}, want_b)


def test_fusion_layer_eval_goes_through_the_same_builder(calls):
    n, Lq, Hd = 2, 5, 64
    layer = _layer(Hd)
    x = torch.zeros((n * Lq, Hd), dtype=bf16)
    y, (pre2, mean2, rstd2, gamma2, beta2), qkv = E.bert_layer_eval_c(x, None, layer, None, n, Lq)
    d = _read(K.BL_FWD, calls["bert_layer_fwd"])
    _check({k: d[k] for k in ("x", "y", "qkv", "pre2", "mean2", "rstd2", "ln2_gamma", "ln2_beta")},
           _ptrs(x=x, y=y, qkv=qkv, pre2=pre2, mean2=mean2, rstd2=rstd2, ln2_gamma=gamma2, ln2_beta=beta2))
    _check({k: d[k] for k in E._BL_PARAMS}, _layer_param_fields(layer))
    zero = ("lse", "h_pre", "key_mask", "res_pre", "res_mean", "res_rstd", "res_gamma", "res_beta", "seed_attn", "seed1", "seed2", "causal_from")
    assert all(d[k] == 0 for k in zero) and d["p_hidden"] == 0 and d["p_attn"] == 0 and d["mean1"] and d["rstd1"]


# ---- Swin block ---------------------------------------------------------------------------------------------------------------------------------
def _block_param_fields(blk):
    a, mlp = blk.attn, blk.mlp
    return _ptrs(ln1_gamma=blk.norm1.weight, ln1_beta=blk.norm1.bias, w_qkv=a.qkv.weight._lav16, b_qkv=a.qkv.bias, w_proj=a.proj.weight._lav16,
                 b_proj=a.proj.bias, ln2_gamma=blk.norm2.weight, ln2_beta=blk.norm2.bias, w_fc1=mlp.fc1.weight._lav16, b_fc1=mlp.fc1.bias,
                 w_fc2=mlp.fc2.weight._lav16, b_fc2=mlp.fc2.bias)


def _block_bwd_fields(blk):
    a, mlp = blk.attn, blk.mlp
    wt = dict(qkv=a.qkv.weight._lav16t, proj=a.proj.weight._lav16t, fc1=mlp.fc1.weight._lav16t, fc2=mlp.fc2.weight._lav16t)
    want = {f"wt_{k}": t.data_ptr() for k, t in wt.items()}
    want.update({f"ldt_{k}": t.stride(0) for k, t in wt.items()})
    want.update(_ptrs(g_ln1_gamma=blk.norm1.weight._lavg, g_ln1_beta=blk.norm1.bias._lavg, g_w_qkv=a.qkv.weight._lavg, g_b_qkv=a.qkv.bias._lavg,
                      g_bias_table=a.relative_position_bias_table._lavg, g_w_proj=a.proj.weight._lavg, g_b_proj=a.proj.bias._lavg,
                      g_ln2_gamma=blk.norm2.weight._lavg, g_ln2_beta=blk.norm2.bias._lavg, g_w_fc1=mlp.fc1.weight._lavg, g_b_fc1=mlp.fc1.bias._lavg,
                      g_w_fc2=mlp.fc2.weight._lavg, g_b_fc2=mlp.fc2.bias._lavg))
    return want


@pytest.mark.parametrize("drop_path", (False, True))
def test_swin_block_descriptors_hold_every_tensor_in_its_named_field(calls, monkeypatch, drop_path):
    M, Cn = 16, 32
    blk = _block(Cn)
    att = NS(d=L.AttnDesc(), lse_elems=lambda: 64)                          # the window descriptor's tables are device work: a stand-in
    monkeypatch.setattr(E, "_window_attn", lambda blk, geo, C_, grid: (att, True))
    geo = dict(B=2, D=1, H=2, W=4, window=(1, 2, 2), shift=(0, 0, 0), cfg_window=(1, 2, 2), arena=object())
    x = torch.zeros((M, Cn), dtype=bf16)
    dp_attn, dp_mlp = (torch.ones(2), torch.ones(2)) if drop_path else (None, None)
    ctx = _Ctx()
    out = E.SwinBlockFn._forward_c(ctx, x, blk, geo, dp_attn, dp_mlp, True)
    assert ctx.att is att                                                   # kept alive for the backward: its address is in the descriptor

    def forward_fields(t):
        xs, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h, da, dm = t
        want = dict(rows=M, C=Cn, heads=1, rows_per_group=M // 2, qkv_headmajor=1, ln_eps=1e-5, attn=C.addressof(att.d), out=out.data_ptr())
        want.update(_block_param_fields(blk))
        want.update(_ptrs(dp_attn=da if drop_path else None, dp_mlp=dm if drop_path else None, x=xs, y1=y1, mean1=st[0], rstd1=st[1], mean2=st[2],
                          rstd2=st[3], qkv=qkv, ao=ao, lse=lse, x_mid=x_mid, y2=y2, h_pre=h_pre, h=h))
        return want

    fwd = _read(K.SB_FWD, calls["swin_block_fwd"])
    _check(fwd, forward_fields(ctx.saved_tensors))
    assert (fwd["dp_attn"] == 0) == (not drop_path) and (fwd["dp_mlp"] == 0) == (not drop_path)
    assert ctx.saved_tensors[2].shape == (4, M) and [fwd[k] - fwd["mean1"] for k in ("rstd1", "mean2", "rstd2")] == [4 * M, 8 * M, 12 * M]

    for moved in (False, True):
        if moved:
            ctx.move()
        dy = torch.zeros((M, Cn), dtype=bf16)
        E.SwinBlockFn._backward_c(ctx, dy)
        bwd = _read(K.SB_BWD, calls["swin_block_bwd"])
        want_f = forward_fields(ctx.saved_tensors) if moved else fwd
        assert not moved or want_f["x"] != fwd["x"]
        _check({k: bwd[k] for k in K.SB_FWD.names}, want_f)
        rest = {k: v for k, v in bwd.items() if k not in K.SB_FWD.pos}
        alpha = 1.0 / 0.8 if drop_path else 1.0
        want_b = _block_bwd_fields(blk)
        want_b.update(dy=dy.data_ptr(), alpha_attn=alpha, alpha_mlp=alpha, assign_mask=0,
                      group_splits=K.group_splits_for(((Cn, 4 * Cn), (4 * Cn, Cn), (Cn, Cn), (3 * Cn, Cn)), M),
                      splits_qkv=K.splits_for(3 * Cn, Cn, M), splits_proj=K.splits_for(Cn, Cn, M, drop_path),
                      splits_fc1=K.splits_for(4 * Cn, Cn, M), splits_fc2=K.splits_for(Cn, 4 * Cn, M, drop_path))
        grads = ("dh", "d_y2", "d_mid", "d_ao", "dqkv", "d_y1", "dx")
        assert all(rest[g] for g in grads) and len({rest[g] for g in grads}) == len(grads)
        _check({k: v for k, v in rest.items() if k not in grads}, want_b)


def test_forward_without_kept_activations_leaves_their_fields_null(calls, monkeypatch):
    blk = _block(32)
    att = NS(d=L.AttnDesc(), lse_elems=lambda: 64)
    monkeypatch.setattr(E, "_window_attn", lambda blk, geo, C_, grid: (att, False))
    geo = dict(B=1, D=1, H=4, W=4, window=(1, 2, 2), shift=(0, 0, 0), cfg_window=(1, 2, 2), arena=None)
    E.SwinBlockFn._forward_c(_Ctx(), torch.zeros((16, 32), dtype=bf16), blk, geo, None, None, False)
    d = _read(K.SB_FWD, calls["swin_block_fwd"])
    assert all(d[k] == 0 for k in ("mean1", "rstd1", "mean2", "rstd2", "lse", "h_pre", "dp_attn", "dp_mlp", "qkv_headmajor")) and d["y1"] and d["out"]


# ---- a changed struct ----------------------------------------------------------------------------------------------------------------------------
def _with_field_inserted(st, name, **override):
    fields = [(n, override.get(n, ct)) for n, ct in st._fields_]
    fields.insert(len(fields) // 2, (name, L.vp))
    return type("Shifted" + st.__name__, (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("stage", ("swin", "bert"))
def test_a_field_inserted_into_a_struct_moves_no_value_into_a_wrong_field(stage):
    """no literal position survives in the engine: its labelled values land by name in a declaration that has grown in the middle (forward and
    backward part), and unlabelled fields read 0"""
    fwd_st, bwd_st, names, n_fwd = ((L.SwinBlockDesc, L.SwinBlockBwdDesc, E._SB_BWD_NAMES, len(E._SB_FWD_NAMES)) if stage == "swin" else
                                    (L.BertLayerDesc, L.BertLayerBwdDesc, E._BL_BWD_NAMES, len(E._BL_FWD_NAMES)))
    real = K.DescLayout(bwd_st)
    assert real.names == (K.SB_BWD if stage == "swin" else K.BL_BWD).names
    shifted = K.DescLayout(_with_field_inserted(bwd_st, "new_bwd", f=_with_field_inserted(fwd_st, "new_fwd")))
    assert len(shifted.names) == len(real.names) + 2 and shifted.pos["new_fwd"] < shifted.pos["dy"] < shifted.pos["new_bwd"]
    vals = tuple((0.5 + i) if ct is L.f32 else (0x3000_0000_0000 + 8 * i) if ct is L.vp else (900 + i)
                 for i, ct in enumerate(dict(K.DescLayout._flatten(bwd_st)[0])[n] for n in names))
    want = dict(zip(names, vals))
    _check(_read(real, real.placer(names)(vals)), want)
    _check(_read(shifted, shifted.placer(names, partial=True)(vals)), dict(want, new_fwd=0, new_bwd=0))
    with pytest.raises(AssertionError):
        shifted.placer(names)                                               # a field nobody fills is an error unless asked for
    fwd_layout = K.DescLayout(_with_field_inserted(fwd_st, "new_fwd"))
    _check(_read(fwd_layout, fwd_layout.placer(names[:n_fwd], partial=True)(vals[:n_fwd])), dict(list(want.items())[:n_fwd], new_fwd=0))


# ---- parameter constants -----------------------------------------------------------------------------------------------------------------------
def test_layer_and_block_constants_are_the_named_addresses_cached_per_arena():
    layer = _layer()
    c = E._layer_consts(layer)
    assert dict(zip(E._BL_PARAMS, c["params"])) == _layer_param_fields(layer)
    assert dict(zip(E._BL_BWD_CONSTS, c["bwd"])) == _layer_bwd_fields(layer)
    a = layer.arena
    assert all(t is u for t, u in zip((c["wqkv16"], c["gwqkv"], c["bqkv"], c["gbqkv"]), (a.w[0], a.w[1], a.b[2], a.b[1])))
    assert (c["eps"], c["eps2"], c["ffn"], c["heads"]) == (1e-12, 1e-11, 128, 1)
    assert E._layer_consts(layer) is c
    layer.arena = _Arena(64)                                                # another arena: other fused views, so the cache is rebuilt
    c2 = E._layer_consts(layer)
    assert c2 is not c and dict(zip(E._BL_PARAMS, c2["params"])) == _layer_param_fields(layer) and c2["params"] != c["params"]

    blk, arena = _block(), object()
    b = E._block_consts(blk, arena)
    assert dict(zip(E._SB_PARAMS, b["params"])) == _block_param_fields(blk)
    assert dict(zip(E._SB_BWD_CONSTS, b["bwd"])) == _block_bwd_fields(blk)
    assert E._block_consts(blk, arena) is b and E._block_consts(blk, object()) is not b
