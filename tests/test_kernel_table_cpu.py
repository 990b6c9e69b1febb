"""CPU: the kernel tables of csrc/kernel_table.h, read through dd_dev_kernel_table, and the *_supported predicates that ask them which
instantiations exist, read through dd_dev_kernel_supported.  Neither needs a context or a GPU.  (That a launch asking for more LDS than its
entry's ceiling is refused before anything touches a device is checked by a stand-alone host program, tools/kernel_table_guard.hip.)"""
import ctypes
from collections import Counter
from itertools import product

import pytest

from duodiff_amd import _lib

# entries per family, as the symbol list of the device code has them (tools/kernel_isa_diff.py)
COUNTS = {"mlp_fused_kernel": 23, "skip_rows_ln_kernel": 4, "qkv_rows_kernel": 3, "head_dec_kernel": 37, "embed_mfma_kernel": 4,
          "qkv_attention_kernel": 3, "v_identity_kernel": 3, "attention_kernel": 4, "attention_long_kernel": 2, "gemm_kernel": 15,
          "gemm256_kernel": 6, "rowlin768_kernel": 1}
LDS_PER_CU = 160 * 1024     # gfx950

WIDTHS = range(32, 1281, 32)
# the shipped configs: embed_dim 512 / 768 / 1024 with 8 / 12 / 16 heads, mlp_ratio 4, 256 patches + 1 or 2 extra tokens,
# (patch, channels, image side) = (4, 3, 64), (2, 3, 32), (2, 4, 32)
HIDDEN = sorted({h + d for h in (2048, 3072, 4096) for d in (-64, -32, 0, 32, 64)} | {0, 32, 64, 96, 128})
ROWLIN_K = sorted({k + d for k in (768, 1536, 3072) for d in (-64, -32, 0, 32, 64)} | {64, 128, 160, 192, 224, 256})
HEADS = sorted({h + d for h in (8, 12, 16) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def table(lib):
    rows, fam, key, block, lds = [], ctypes.create_string_buffer(32), (ctypes.c_int * 4)(), ctypes.c_int(), ctypes.c_int()
    while (rc := lib.dd_dev_kernel_table(len(rows), fam, key, ctypes.byref(block), ctypes.byref(lds))) == 0:
        rows.append((fam.value.decode(), tuple(key), block.value, lds.value))
        assert len(rows) < 1000
    assert rc == 1
    return rows


def test_keys_are_unique_within_a_family(table):
    dup = [k for k, n in Counter((fam, key) for fam, key, _, _ in table).items() if n > 1]
    assert not dup, dup


def test_block_sizes_are_whole_waves(table):
    assert all(block % 64 == 0 and 64 <= block <= 1024 for _, _, block, _ in table), table


def test_lds_ceilings_fit_a_cu(table):
    assert all(0 < lds <= LDS_PER_CU for _, _, _, lds in table), table      # (the largest: the block tail at embed_dim 512, 161 920 bytes)


def test_entry_counts(table):
    assert Counter(fam for fam, _, _, _ in table) == COUNTS and len(table) == 105
    per_width = Counter((fam, key[0]) for fam, key, _, _ in table)
    assert [per_width[("mlp_fused_kernel", d)] for d in (64, 128, 256, 512)] == [2, 7, 7, 7]
    assert [per_width[("head_dec_kernel", d)] for d in (256, 512, 768, 1024)] == [16, 16, 3, 2]


def _supported(lib, predicate, *args):
    a = (ctypes.c_int * 6)(*args, *([0] * (6 - len(args))))
    rc = lib.dd_dev_kernel_supported(predicate, a)
    assert rc in (0, 1), (predicate, args, rc)
    return bool(rc)


def test_mlp_fused_supported_is_the_parents_rule(lib):
    for D, hidden in product(WIDTHS, HIDDEN):
        want = D in (64, 128, 256, 512) and hidden % 64 == 0 and 64 <= hidden <= 4096
        assert _supported(lib, _lib.DD_DEV_SUP_MLP_FUSED, D, hidden) == want, (D, hidden)


def test_head_dec_supported_is_the_parents_rule(lib):
    for D, pd in product(WIDTHS, range(0, 69)):
        nt = (pd + 15) // 16
        want = 1 <= pd <= 64 and pd % 4 == 0 and (D in (256, 512) or (D == 768 and nt <= 3) or (D == 1024 and nt <= 2))
        assert _supported(lib, _lib.DD_DEV_SUP_HEAD_DEC, D, pd) == want, (D, pd)
    for D in WIDTHS:
        assert _supported(lib, _lib.DD_DEV_SUP_HEAD_DEC_PROBE, D) == (D in (256, 512)), D


def test_qkv_attention_supported_is_the_parents_rule(lib):
    for D, extras, dl in product(WIDTHS, range(0, 4), (-1, 0, 1)):
        L = 256 + extras + dl
        for H in sorted(set(HEADS) | {D // 64}):
            want = D in (512, 768, 1024) and H * 64 == D and extras in (1, 2) and L == 256 + extras
            assert _supported(lib, _lib.DD_DEV_SUP_QKV_ATTENTION, D, H, L, extras) == want, (D, H, L, extras)


def test_rowlin_supported_is_the_parents_rule(lib):
    for D, K in product(WIDTHS, ROWLIN_K):
        want = D == 768 and K % 64 == 0 and K >= 192
        assert _supported(lib, _lib.DD_DEV_SUP_ROWLIN, D, K) == want, (D, K)


def test_embed_predicates_are_the_parents_rules(lib):
    for D, P, C, ds, extras, dl in product(WIDTHS, range(1, 6), range(2, 6), (-1, 0, 1), range(0, 4), (-1, 0, 1)):
        S, L, pd = 16 * P + ds, 256 + extras + dl, C * P * P
        lds = (D // 32) * 2 * ((pd // 4 + 3) // 4) * 1024
        mfma = (S == 16 * P and D % 32 == 0 and pd % 4 == 0 and lds <= 156 * 1024 and L == extras + 256
                and (P, C) in ((4, 3), (2, 3), (2, 4)))
        assert _supported(lib, _lib.DD_DEV_SUP_EMBED_MFMA, P, C, D, S, L, extras) == mfma, (P, C, D, S, L, extras)
        assert _supported(lib, _lib.DD_DEV_SUP_EMBED_LN, P, C, D, S, L, extras) == (mfma and P == 4 and C == 3 and D == 512), (P, C, D, S, L, extras)


def test_an_over_large_request_is_refused_before_the_launch(tmp_path):
    """tools/kernel_table_guard.hip: kernel_table.h with a dummy kernel and its own main, built and run on the host"""
    import subprocess
    from conftest import REPO
    from duodiff_amd.build import ARCH, CSRC, hipcc
    exe = tmp_path / "guard"
    subprocess.run([hipcc(), "-std=c++20", f"--offload-arch={ARCH}", f"-I{CSRC}", str(REPO / "tools" / "kernel_table_guard.hip"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("ok: ") == 7 and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_an_unknown_predicate_is_refused(lib):
    assert lib.dd_dev_kernel_supported(99, (ctypes.c_int * 6)()) == _lib.DD_ERR_INVALID
    assert lib.dd_dev_kernel_supported(_lib.DD_DEV_SUP_ROWLIN, None) == _lib.DD_ERR_INVALID
