"""Real early exit, the parts that need no device: the block-row count, the hole-fill plan of a compaction (the host function beside
the decision kernel, through the library) and the binding's argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

from duodiff_amd.early_exit import real_exit_block_rows


def test_block_rows_by_hand():
    # depth 3: an image with exit index e runs the blocks in front of the first compaction layer at or behind e
    assert real_exit_block_rows([0, 1, 2, 3], 3, 1) == 0 + 1 + 2 + 3
    assert real_exit_block_rows([0, 1, 2, 3], 3, 2) == 0 + 2 + 2 + 3          # layers 0 and 2 compact
    assert real_exit_block_rows([0, 1, 2, 3], 3, 3) == 0 + 3 + 3 + 3          # layer 0 alone
    assert real_exit_block_rows([0, 1, 2, 3], 3, 4) == 0 + 3 + 3 + 3
    assert real_exit_block_rows(np.full((7, 5), 13), 13, 1) == 7 * 5 * 13     # nobody leaves
    assert real_exit_block_rows(np.zeros((7, 5)), 13, 4) == 0                 # everybody leaves at layer 0
    assert real_exit_block_rows([5, 9, 12], 13, 4) == 8 + 12 + 12
    assert real_exit_block_rows([], 13, 1) == 0
    for bad in (lambda: real_exit_block_rows([0], 3, 0), lambda: real_exit_block_rows([4], 3, 1), lambda: real_exit_block_rows([-1], 3, 1)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("depth,s", [(3, 1), (3, 2), (3, 4), (13, 1), (13, 2), (13, 4), (13, 14), (5, 5)])
def test_block_rows_against_a_restatement(depth, s):
    """brute force: walk the layers; a compaction layer drops the images whose exit index it has reached"""
    rng = np.random.default_rng(depth * 100 + s)
    idx = rng.integers(0, depth + 1, size=(11, 9))
    rows = 0
    for e in idx.ravel():
        running = True
        for l in range(depth):
            if l % s == 0 and e <= l:
                running = False
            rows += running
    assert real_exit_block_rows(idx, depth, s) == rows


def _plan(alive):
    from duodiff_amd import _lib as L
    lib = L.load()
    n = len(alive)
    a = (C.c_int * max(n, 1))(*[int(v) for v in alive])
    keep, n_moves = C.c_int(-1), C.c_int(-1)
    moves = (C.c_int * (2 * (n // 2) + 2))()
    assert lib.dd_dev_ee_real_plan(a, n, C.byref(keep), C.byref(n_moves), moves) == L.DD_OK
    return keep.value, [(moves[2 * k], moves[2 * k + 1]) for k in range(n_moves.value)]


def _masks(n):
    yield "none", [1] * n
    yield "all", [0] * n
    yield "alternating", [i % 2 for i in range(n)]
    yield "alternating'", [(i + 1) % 2 for i in range(n)]
    yield "tail-only", [1] * (n - n // 3 - 1) + [0] * (n // 3 + 1)      # the leavers sit at the end: nothing to move
    yield "head-only", [0] * (n // 3 + 1) + [1] * (n - n // 3 - 1)      # the leavers sit in front
    rng = np.random.default_rng(n)
    for k in range(4):
        yield f"random{k}", [int(v) for v in rng.integers(0, 2, n)]


@pytest.mark.parametrize("n", [1, 2, 7, 128])
def test_hole_fill_plan(n):
    for name, alive in _masks(n):
        keep, moves = _plan(alive)
        assert keep == sum(alive), name
        srcs, dsts = [m[0] for m in moves], [m[1] for m in moves]
        holes = [d for d in range(keep) if not alive[d]]
        assert dsts == holes, f"{name}: the holes of the prefix, in increasing order"
        assert srcs == [q for q in range(keep, n) if alive[q]], f"{name}: the survivors behind the prefix, in increasing order"
        assert not set(srcs) & set(dsts) and all(s >= keep > d for s, d in moves), f"{name}: sources and destinations are disjoint"
        # carry the moves out on the slot -> image table, as the decision kernel does: the image that left takes the vacated slot
        tab = list(range(n))
        for s, d in moves:
            tab[d], tab[s] = tab[s], tab[d]
        assert sorted(tab) == list(range(n)), f"{name}: the table stays a permutation"
        assert all(alive[tab[q]] for q in range(keep)) and not any(alive[tab[q]] for q in range(keep, n)), f"{name}: the prefix is dense"
        if name in ("none", "all", "tail-only"):
            assert moves == [], name
        if name == "head-only" and keep:
            assert len(moves) == min(n - keep, keep)


def test_hole_fill_plan_every_mask_of_length_7():
    for alive in itertools.product((0, 1), repeat=7):
        keep, moves = _plan(alive)
        tab = list(range(7))
        for s, d in moves:
            assert s >= keep > d
            tab[d], tab[s] = tab[s], tab[d]
        assert keep == sum(alive) and all(alive[tab[q]] for q in range(keep)) and len(moves) == sum(1 for d in range(keep) if not alive[d])


def test_binding_argument_checks_without_a_device():
    from duodiff_amd import _lib as L
    from duodiff_amd.engine import sample_early_exit_real_loop
    lib = L.load()
    assert set(f[0] for f in L.dd_ee_real._fields_) == {"compact_every", "reserved"} and C.sizeof(L.dd_ee_real) == 8
    # no context: refused before anything is touched
    args, real = L.dd_ee_sample_args(), L.dd_ee_real(1, 0)
    assert lib.dd_sample_early_exit_real(None, C.byref(args), C.byref(real), None) == L.DD_ERR_INVALID
    assert lib.dd_dev_ee_real_stats(None, (C.c_longlong * 3)()) == L.DD_ERR_INVALID
    assert lib.dd_dev_ee_real_plan(None, 0, None, None, None) == L.DD_ERR_INVALID
    # the Python entry refuses before it reads the context, the model or the tensors
    with pytest.raises(ValueError, match="compact_every"):
        sample_early_exit_real_loop(None, None, None, 0.1, compact_every=0)
    with pytest.raises(ValueError, match="compact_every"):
        sample_early_exit_real_loop(None, None, None, 0.1, compact_every=1.5)
    with pytest.raises(ValueError, match="err must be None"):
        sample_early_exit_real_loop(None, None, None, 0.1, err=object())
    with pytest.raises(ValueError, match="noise"):
        sample_early_exit_real_loop(None, None, None, 0.1, noise="torch_cpu")


def test_cli_flags():
    from duodiff_amd import eesampler
    base = ["--threshold", "0.1", "--checkpoint_path", "x", "--batch_size", "2", "--output_folder", "o", "--config_path", "c"]
    a = eesampler.get_args(base + ["--real_exit", "--compact_every", "4"])
    assert a.real_exit and a.compact_every == 4
    a = eesampler.get_args(base)
    assert not a.real_exit and a.compact_every == 1
    for bad in (["--compact_every", "2"], ["--real_exit", "--compact_every", "0"]):
        with pytest.raises(SystemExit):
            eesampler.get_args(base + bad)
