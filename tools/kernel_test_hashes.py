"""pytest plugin for bit-identity runs of the per-element kernel tests against two builds of the library:

    DUODIFF_LIB=/path/to/other/libduodiff.so KERNEL_TEST_HASHES=a.txt PYTHONPATH=tools python -m pytest -p kernel_test_hashes -m gpu tests/test_attention.py ...
    KERNEL_TEST_HASHES=b.txt PYTHONPATH=tools python -m pytest -p kernel_test_hashes -m gpu ...      then      cmp a.txt b.txt

One sha256 per test (shapes and dtypes hashed with the bytes) over every array the test hands to tests/kernel_support.py gate() as `got`, and over every
array of more than one element (single elements: timings) it hands to an entry point through kernel_support.P -- inputs and outputs whole, canary rows
included, as they are when the test is over.  The tests' operands are seeded, so equal libraries give equal files.  Changes no test."""
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for _p in (str(REPO), str(REPO / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import kernel_support  # noqa: E402  (before the test modules import gate / P from it)

_gate, _P = kernel_support.gate, kernel_support.P
_cur = {"h": None, "n": 0}
_arrays, _lines = [], []


def _add(a):
    a = np.ascontiguousarray(a)
    _cur["h"].update(str(a.shape).encode() + str(a.dtype).encode() + a.tobytes())
    _cur["n"] += 1


def gate(got, want, tol, what):
    if _cur["h"] is not None:
        _add(np.asarray(got))
    return _gate(got, want, tol, what)


def P(a):
    if a is not None and _cur["h"] is not None and a.size > 1:
        _arrays.append(a)
    return _P(a)


kernel_support.gate, kernel_support.P = gate, P


def pytest_runtest_setup(item):
    _cur["h"], _cur["n"] = hashlib.sha256(), 0


def pytest_runtest_teardown(item):
    if _cur["h"] is not None:
        for a in _arrays:
            _add(a)
        if _cur["n"]:
            _lines.append(f"{item.nodeid}  {_cur['h'].hexdigest()}  {_cur['n']}")
    _arrays.clear()
    _cur["h"] = None


def pytest_sessionfinish(session):
    out = os.environ.get("KERNEL_TEST_HASHES")
    if out:
        Path(out).write_text("\n".join(_lines) + "\n")
