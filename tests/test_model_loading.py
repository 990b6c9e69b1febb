"""The C-level state_dict contract of a model (dd_model_set_param / dd_model_finalize / dd_model_enable_early_exit), driven through
engine.Model directly: the Python wrappers (uvit.py, early_exit.py) filter names before they reach set_param.  Every key of the Python
schema is accepted; unknown names, wrong shapes, missing keys and calls out of order are refused with the C side's messages."""
import re

import pytest
import torch

from duodiff_amd.config import ModelParams
from duodiff_amd.weights import ee_param_shapes, num_params, param_shapes

from conftest import TINY

CTYPES = ["mlp_probe_per_layer", "mlp_probe_per_timestep", "mlp_probe_per_layer_per_timestep", "attention_probe"]


def _model(cfg, ctype=None):
    from duodiff_amd.engine import Context, Model
    m = Model(Context.get(), ModelParams.from_dict(cfg), 2)
    if ctype:
        m.enable_early_exit(ctype)
    return m


def _schema(cfg, ctype=None):
    """name -> shape of what the engine model is given (EarlyExitUViT.engine_model strips the uvit. prefix)"""
    mp = ModelParams.from_dict(cfg)
    if ctype is None:
        return dict(param_shapes(mp))
    return {k[len("uvit."):] if k.startswith("uvit.") else k: v for k, v in ee_param_shapes(mp, ctype).items()}


def _load(m, shapes, skip=None):
    for name, shp in shapes.items():
        if name != skip:
            m.set_param(name, torch.full(shp, 0.01))


def _num_params(m):
    return m.ctx.lib.dd_model_num_params(m.handle)


def _elems(shapes):
    return sum(torch.Size(s).numel() for s in shapes.values())


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{}, dict(num_classes=10), dict(qkv_bias=True), dict(mlp_time_embed=True)],
                         ids=["plain", "cond", "qkv_bias", "time_mlp"])
def test_every_plain_key_is_accepted(extra):
    cfg = dict(TINY, **extra)
    shapes = _schema(cfg)
    m = _model(cfg)
    _load(m, shapes)
    assert _num_params(m) == _elems(shapes) == num_params(ModelParams.from_dict(cfg))
    m.finalize()
    assert _num_params(m) == 0          # the host copies are dropped


@pytest.mark.gpu
@pytest.mark.parametrize("ctype", CTYPES)
def test_every_early_exit_key_is_accepted(ctype):
    shapes = _schema(dict(TINY), ctype)
    m = _model(dict(TINY), ctype)
    _load(m, shapes)
    assert _num_params(m) == _elems(shapes)
    m.finalize()
    assert _num_params(m) == 0


def _rejects(m, name, shape=(64,)):
    with pytest.raises(KeyError, match=re.escape(f"unexpected key in state_dict: {name}")):
        m.set_param(name, torch.zeros(shape))


@pytest.mark.gpu
def test_unknown_names_are_rejected():
    half = TINY["depth"] // 2
    plain = _model(dict(TINY))
    for name in ["in_blocks.0.skip_linear.weight", "mid_block.skip_linear.bias", f"in_blocks.{half}.norm1.weight",
                 f"out_blocks.{half}.norm1.weight", "label_emb.weight", "in_blocks.0.attn.qkv.bias", "time_embed.0.weight",
                 "in_blocks_heads.0.norm.weight", "mid_block_head.decoder_pred.bias", "matrix.0.classifier.0.weight", "no_such_key"]:
        _rejects(plain, name)
    _rejects(_model(dict(TINY), "mlp_probe_per_layer"), f"matrix.{TINY['depth']}.classifier.0.weight", (1, 64))
    _rejects(_model(dict(TINY), "mlp_probe_per_timestep"), "matrix.1000.classifier.0.weight", (1, 64))
    _rejects(_model(dict(TINY), "mlp_probe_per_layer_per_timestep"), "matrix.0, 1000.classifier.0.weight", (1, 64))
    _rejects(_model(dict(TINY), "attention_probe"), "matrix.0.classifier.0.weight", (1, 64))


@pytest.mark.gpu
def test_wrong_shapes_are_rejected():
    m = _model(dict(TINY), "mlp_probe_per_layer")
    pd = TINY["patch_size"] ** 2 * TINY["in_chans"]
    for name, bad, want in [("in_blocks.0.attn.qkv.weight", (64, 64), "[192,64]"), ("pos_embed", (1, 64), "[1,17,64]"),
                            ("mid_block_head.decoder_pred.weight", (pd, 32), f"[{pd},64]"), ("matrix.0.classifier.0.weight", (64,), "[1,64]")]:
        got = "[" + ",".join(map(str, bad)) + "]"
        with pytest.raises(ValueError, match=re.escape(f"size mismatch for {name}: expected {want}, got {got}")):
            m.set_param(name, torch.zeros(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("ctype,missing", [(None, "norm.weight"), ("mlp_probe_per_layer", "out_blocks.0.skip_linear.bias"),
                                           ("mlp_probe_per_layer", "out_blocks_heads.0.final_layer.bias"),
                                           ("mlp_probe_per_layer_per_timestep", "matrix.2, 999.classifier.0.bias"),
                                           ("attention_probe", "matrix.1.weight_kv.weight")])
def test_finalize_names_the_missing_key(ctype, missing):
    shapes = _schema(dict(TINY), ctype)
    assert missing in shapes
    m = _model(dict(TINY), ctype)
    _load(m, shapes, skip=missing)
    with pytest.raises(KeyError, match=re.escape(f"missing key in state_dict: {missing}")):
        m.finalize()


@pytest.mark.gpu
def test_calls_out_of_order_are_refused():
    m = _model(dict(TINY))
    m.set_param("norm.weight", torch.ones(64))
    with pytest.raises(RuntimeError, match="enable early exit before any parameter is set"):
        m.enable_early_exit("mlp_probe_per_layer")
    shapes = _schema(dict(TINY))
    _load(m, shapes)
    m.finalize()
    with pytest.raises(RuntimeError, match="model already finalized"):
        m.set_param("norm.weight", torch.ones(64))
    with pytest.raises(RuntimeError, match="enable early exit before any parameter is set"):
        m.enable_early_exit("mlp_probe_per_layer")
