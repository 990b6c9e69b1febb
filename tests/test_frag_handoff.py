"""The patch rows' hand-offs in MFMA fragment order at embed_dim 512: attention output -> projection (ao_frag), in-block
copy -> the out-block's skip_linear (out_frag / skip_frag), residual rows from one block tail to the next (x_in_frag / x_out_frag).

All three are pure re-addressing: a kernel moves the same registers to other addresses, so every comparison here is exact equality of bits.
  * kernel level: each launch once row-major (dd_dev_qkv_attention_rows, dd_dev_block_tail) and once in fragment form (dd_dev_qkv_attention_frag,
    dd_dev_block_tail_frag) on the same seeded operands; the fragment buffers are un-permuted with the index maps of tests/kernel_support.py, which are
    written from the layout definitions alone; the canary rows around every fragment output and every row a launch must leave alone keep their bytes.
  * model level: a depth-3 width-512 model (in-block: row-major -> fragment, mid block: fragment -> fragment with the skip read, out block:
    fragment -> row-major) with each stage switched off by its development flag, in one chain and in two.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_support
from duodiff_amd import _lib as L
from kernel_support import P, bf16, bf16_bits, frag16_index, frag32_index, round_up, to_frag, unfrag
from loop_support import QA512, ddpm_rows, dev_flags, ee_uvit, images, run_loop, side_stream, uvit

gpu = pytest.mark.gpu

D, H, N = 512, 8, 256
HIDDEN = 64                    # the smallest hidden size mlp_fused_supported accepts (two chunks: the skip phases need an even count)
POISON = 0xFF
ALL_OFF = L.DD_DEV_NO_FRAG_AO | L.DD_DEV_NO_FRAG_SKIP | L.DD_DEV_NO_FRAG_X


# ---------------------------------------------------------------------------------------------------------------- the layouts
def test_index_maps_are_bijections_and_agree_with_the_norm1_fragment_order():
    rows = 96
    for idx in (frag16_index(rows, D), frag32_index(rows, D)):
        assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(rows * D))
    a = np.arange(rows * D, dtype=np.uint16).reshape(rows, D)
    f = a.reshape(rows // 32, 32, D // 16, 2, 8).transpose(0, 2, 3, 1, 4).reshape(-1)      # MlpFusedArgs::ln_out_frag: [grp][ks][lane >> 5][lane & 31][i]
    assert np.array_equal(to_frag(a, D), f)
    assert np.array_equal(unfrag(f, rows // 32, D), a)
    # one wave instruction (fixed group, k-step or (t, g)) covers 1 KB contiguous
    i16, i32 = frag16_index(32, D), frag32_index(32, D)
    assert set((i16[:, 16:32].reshape(-1) * 2) // 1024) == {1} and set((i32[:, 40:48].reshape(-1) * 4) // 1024) == {5}


def test_lib_binds_the_fragment_entry_points_and_flags():
    assert {"dd_dev_block_tail_frag", "dd_dev_qkv_attention_frag"} <= set(L.SIGNATURES)
    assert len(L.SIGNATURES["dd_dev_block_tail_frag"][1]) == len(L.SIGNATURES["dd_dev_block_tail"][1]) + 5
    hdr = (L.LIB_PATH.parent.parent / "include" / "duodiff_dev.h").read_text()
    for name in ("DD_DEV_NO_FRAG_AO", "DD_DEV_NO_FRAG_SKIP", "DD_DEV_NO_FRAG_X"):
        assert f"#define {name} {getattr(L, name)}u" in hdr


# ---------------------------------------------------------------------------------------------------------------- helpers
def all_bytes(a, byte):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == byte))


# ---------------------------------------------------------------------------------------------------------------- the attention launch
@gpu
@pytest.mark.parametrize("B,E", [(2, 1), (3, 2)])
def test_attention_output_in_fragment_order(B, E):
    ctx = kernel_support.ctx()
    Lt, M = N + E, B * (N + E)
    r = np.random.default_rng([B, E, 1])
    h = r.standard_normal((M, D)).astype(np.float32)
    w = (0.05 * r.standard_normal((3 * D, D))).astype(np.float32)
    xres = r.standard_normal((M, D)).astype(np.float32)
    ln = np.stack([1.0 + 0.2 * r.standard_normal(D), 0.1 * r.standard_normal(D)]).astype(np.float32)
    want = np.zeros((M + 8, D), np.uint16)
    ctx.check(ctx.lib.dd_dev_qkv_attention_rows(ctx.handle, B, Lt, H, E, P(h), P(w), None, P(xres), P(ln), P(want), 0, None, C.byref(C.c_float(0))))
    got = np.zeros((M + 8, D), np.uint16)
    frag = np.zeros((B * N + 16) * D, np.uint16)
    ctx.check(ctx.lib.dd_dev_qkv_attention_frag(ctx.handle, B, Lt, H, E, P(h), P(w), None, P(xres), P(ln), P(got), P(frag), 0, None, C.byref(C.c_float(0))))
    patch = (np.arange(M) % Lt) >= E
    assert np.isfinite((want[:M].astype(np.uint32) << 16).view(np.float32)).all()
    assert np.array_equal(unfrag(frag[8 * D:], B * N // 32, D), want[:M][patch]), "patch rows: the fragment buffer un-permuted differs from the row-major launch"
    assert all_bytes(frag[: 8 * D], 0xFF) and all_bytes(frag[8 * D + B * N * D:], 0xFF), "canary rows around out_frag"
    assert np.array_equal(got[:M][~patch], want[:M][~patch]), "extra-token rows still go to the row-major buffer"
    assert all_bytes(got[:M][patch], 0xFF), "the row-major patch rows must not be written"
    assert all_bytes(got[M:], 0xFF) and all_bytes(want[M:], 0xFF)


# ---------------------------------------------------------------------------------------------------------------- the block tail
class TailOps:
    def __init__(self, B, E):
        self.B, self.E, self.L, self.M = B, E, N + E, B * (N + E)
        r = np.random.default_rng([B, E, 2])
        M = self.M
        self.x = r.standard_normal((M, D)).astype(np.float32)
        self.ao = bf16(r.standard_normal((M, D)))
        self.skip = bf16(r.standard_normal((M, D)))
        self.w1 = (0.05 * r.standard_normal((HIDDEN, D))).astype(np.float32)
        self.b1 = r.standard_normal(HIDDEN).astype(np.float32)
        self.w2 = (0.1 * r.standard_normal((D, HIDDEN))).astype(np.float32)
        self.b2 = (0.2 * r.standard_normal(D)).astype(np.float32)
        self.wproj = (0.04 * r.standard_normal((D, D))).astype(np.float32)
        self.bproj = (0.2 * r.standard_normal(D)).astype(np.float32)
        self.wskip = (0.04 * r.standard_normal((D, 2 * D))).astype(np.float32)
        self.bskip = (0.2 * r.standard_normal(D)).astype(np.float32)
        self.ln_in = np.stack([1.0 + 0.2 * r.standard_normal(D), 0.1 * r.standard_normal(D)]).astype(np.float32)
        self.ln_out = np.stack([1.0 + 0.2 * r.standard_normal(D), 0.1 * r.standard_normal(D)]).astype(np.float32)
        self.patch = (np.arange(M) % self.L) >= E


_OPS = {}


def tail_ops(B, E):
    if (B, E) not in _OPS:
        _OPS[(B, E)] = TailOps(B, E)
    return _OPS[(B, E)]


# role -> (skip phases, last block's launch, the hand-offs that role can take)
ROLES = {"plain": (False, False, ("ao", "xin", "out", "xout")), "skip": (True, False, ("ao", "skip", "xin", "xout")), "last": (False, True, ("ao", "xin"))}
_REF = {}


def run_tail(o, role, frags):
    """one block tail: the fused launch + the launches of its extra-token rows.  frags = the hand-offs taken in fragment order (empty: the row-major
    launch through dd_dev_block_tail).  Every buffer comes back whole."""
    ctx = kernel_support.ctx()
    skp, last, _ = ROLES[role]
    M, B, E = o.M, o.B, o.E
    Mo = round_up(M, 256) + 8
    pe = B * N * D
    res = {}
    res["xres"] = np.full((Mo, D), 0xFFFFFFFF, np.uint32).view(np.float32)
    res["xres"][:M] = o.x
    res["out"] = None if last else np.zeros((Mo, D), np.uint16)
    res["ln"] = None if last else np.zeros((Mo, D), np.uint16)
    res["hfrag"] = None if last else np.zeros(Mo * D, np.uint16)
    srows = (0 if last else (B * E + 31) // 32) * 16 * 32 + 8
    res["slab"] = np.zeros((srows, D), np.float32)
    plan = (C.c_int * 4)()
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = [None, o.w1, o.b1, o.w2, o.b2, o.ln_in, f32(o.ao), o.wproj, o.bproj, None if last else o.ln_out,
            f32(o.skip) if skp else None, o.wskip if skp else None, o.bskip if skp else None, None]
    common = [ctx.handle, B, N, E, D, HIDDEN, 1 if last else 0, POISON, *[P(a) for a in keep], P(res["xres"]), P(res["out"]), P(res["ln"]), P(res["hfrag"]),
              None, None, P(res["slab"]), srows, C.cast(plan, C.c_void_p), 0, None, C.byref(C.c_float(0))]
    if not frags:
        ctx.check(ctx.lib.dd_dev_block_tail(*common))
        return res
    ins = {"ao": to_frag(bf16_bits(o.ao[o.patch]), D) if "ao" in frags else None,
           "skip": to_frag(bf16_bits(o.skip[o.patch]), D) if "skip" in frags else None,
           "xin": to_frag(o.x[o.patch], D, index=frag32_index) if "xin" in frags else None}
    res["out_frag"] = np.zeros(pe + 16 * D, np.uint16) if "out" in frags else None
    res["xout_frag"] = np.zeros(pe + 16 * D, np.float32) if "xout" in frags else None
    ctx.check(ctx.lib.dd_dev_block_tail_frag(*common, P(ins["ao"]), P(ins["skip"]), P(ins["xin"]), P(res["out_frag"]), P(res["xout_frag"])))
    return res


def ref_tail(o, role):
    key = (o.B, o.E, role)
    if key not in _REF:
        _REF[key] = run_tail(o, role, ())
        assert np.isfinite(_REF[key]["xres"][: o.M][o.patch if ROLES[role][1] else slice(None)]).all()
    return _REF[key]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_tail(o, role, frags):
    want, got = ref_tail(o, role), run_tail(o, role, frags)
    M, pe, pr = o.M, o.B * N * D, o.patch
    for k in ("ln", "hfrag", "slab"):        # norm1 (row-major and in fragment order) and the slabs do not depend on the form of the hand-offs
        if want[k] is not None:
            assert same(got[k], want[k]), f"{role} {frags}: {k} differs"
    # the residual rows
    if "xout" in frags:
        xf = got["xout_frag"]
        assert same(unfrag(xf[8 * D:], o.B * N // 32, D, index=frag32_index), want["xres"][:M][pr]), f"{role} {frags}: x_out_frag un-permuted differs from the row-major rows"
        assert all_bytes(xf[: 8 * D], 0xFF) and all_bytes(xf[8 * D + pe:], 0xFF), "canary rows around x_out_frag"
        if "xin" in frags:       # (the harness poisons the row-major patch rows that x_in_frag stands in for)
            assert all_bytes(got["xres"][:M][pr], POISON), "the row-major patch rows of x must keep their poison bytes"
        else:
            assert same(got["xres"][:M][pr], o.x[pr]), "the row-major patch rows of x must keep their bytes"
    else:
        assert same(got["xres"][:M][pr], want["xres"][:M][pr]), f"{role} {frags}: patch rows of x differ"
    assert same(got["xres"][:M][~pr], want["xres"][:M][~pr]) and same(got["xres"][M:], want["xres"][M:]), f"{role} {frags}: extra-token or canary rows of x differ"
    # the bf16 copy
    if want["out"] is not None:
        if "out" in frags:
            of = got["out_frag"]
            assert same(unfrag(of[8 * D:], o.B * N // 32, D), want["out"][:M][pr]), f"{role} {frags}: out_frag un-permuted differs from the row-major copy"
            assert all_bytes(of[: 8 * D], 0xFF) and all_bytes(of[8 * D + pe:], 0xFF), "canary rows around out_frag"
            assert all_bytes(got["out"][:M][pr], 0xFF), "the row-major patch rows of the copy must not be written"
        else:
            assert same(got["out"][:M][pr], want["out"][:M][pr])
        assert same(got["out"][:M][~pr], want["out"][:M][~pr]) and same(got["out"][M:], want["out"][M:])


@gpu
@pytest.mark.parametrize("B,E", [(2, 1), (3, 2)])
@pytest.mark.parametrize("role", sorted(ROLES))
def test_block_tail_with_every_hand_off_in_fragment_order(role, B, E):
    check_tail(tail_ops(B, E), role, ROLES[role][2])


@gpu
@pytest.mark.parametrize("role,one", [(r, f) for r in sorted(ROLES) for f in ROLES[r][2]])
def test_block_tail_with_one_hand_off_in_fragment_order(role, one):
    """each pointer alone (null = row-major for the others): the first block's tail reads x row-major and writes fragments, the last one the reverse"""
    check_tail(tail_ops(3, 2), role, (one,))


@gpu
def test_block_tail_refuses_fragment_hand_offs_it_has_no_path_for():
    """the skip phases keep y in registers: no bf16 copy of the patch rows exists that could go to out_frag; nothing is launched"""
    with pytest.raises(Exception, match="block tail"):
        run_tail(tail_ops(2, 1), "skip", ("out",))


# ---------------------------------------------------------------------------------------------------------------- the model
STAGES = {"all_frag": 0, "no_ao": L.DD_DEV_NO_FRAG_AO, "no_skip": L.DD_DEV_NO_FRAG_SKIP, "no_x": L.DD_DEV_NO_FRAG_X, "row_major": ALL_OFF}


def _model(flags, B):
    """an engine model finalized under `flags` (the hand-offs are a property of the model, chosen in dd_model_finalize)"""
    m, _ = uvit(QA512, 71, "bf16", max_batch=B)
    with dev_flags(kernel_support.ctx(), flags):
        em = m.engine_model(B)
    return m, em


@gpu
def test_model_outputs_do_not_depend_on_the_form_of_the_hand_offs():
    B = 4
    ctx = kernel_support.ctx()
    x = images(B, 3, 64, 5)
    outs = {}
    for name, flags in STAGES.items():
        m, em = _model(flags, B)
        fwd = em.forward(x, 417.0, None).clone()
        pag = em.forward_perturbed(x[:2], 417.0, None, 0.7, [1]).clone() if name in ("all_frag", "row_major") else None   # identity attention in the mid block
        s = side_stream()
        loops = {}
        for chains, cf in (("two", L.DD_DEV_FORCE_CHAINS), ("one", L.DD_DEV_NO_CHAINS)):
            loops[chains], _, count = run_loop("ddpm", em, x, ddpm_rows(4), s, flags=cf, seed=0)
            assert count == (2 if chains == "two" else 1)
        torch.cuda.synchronize()
        assert torch.isfinite(fwd).all() and torch.isfinite(loops["one"]).all()
        assert torch.equal(loops["one"], loops["two"]), f"{name}: two half-batch chains differ from one chain"
        outs[name] = (fwd, loops["one"], pag)
        del em, m
    base = outs["row_major"]
    for name, (fwd, loop, pag) in outs.items():
        assert torch.equal(fwd, base[0]), f"{name}: dd_forward differs from the row-major model"
        assert torch.equal(loop, base[1]), f"{name}: the 4-step loop differs from the row-major model"
    assert torch.equal(outs["all_frag"][2], base[2]), "a perturbed block (row-major ao on both sides) differs from the row-major model"
    assert not torch.equal(outs["all_frag"][2], outs["all_frag"][0][:2])


@gpu
def test_stale_workspace_bytes_do_not_reach_the_outputs():
    """every fragment buffer is written before it is read: a forward on poisoned workspaces equals the first forward of the model"""
    B = 4
    ctx = kernel_support.ctx()
    m, em = _model(0, B)
    x = images(B, 3, 64, 6)
    first = em.forward(x, 100.0, None).clone()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, em.handle, None))
    torch.cuda.synchronize()
    again = em.forward(x, 100.0, None)
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and torch.equal(first, again)


@gpu
def test_early_exit_model_keeps_the_residual_rows_row_major():
    """the early-exit heads read x every block, so such a model takes ao_frag and the skip hand-off only: the same bits as all row-major"""
    B = 2
    x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    got = {}
    for name, flags in (("frag", 0), ("row_major", ALL_OFF)):
        with dev_flags(kernel_support.ctx(), flags):
            m, mp = ee_uvit(QA512, 73, "mlp_probe_per_layer", "bf16", max_batch=B)
            eps, cls, outs = m(x, torch.full((B,), 300.0), None)
            got[name] = (eps.clone(), torch.stack(cls).clone(), torch.stack(outs).clone())
            torch.cuda.synchronize()
        del m
    for a, b in zip(got["frag"], got["row_major"]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
