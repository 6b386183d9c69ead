"""The greedy screen without a GPU: the float64 restatement's bound (cls_screen_ref.py) holds on the op-level cases, and the header, the export map and
api.py agree on the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import cls_screen_ref as ref
from conftest import ROOT

SEED = 4242
NEW = ("q4_set_greedy_screen", "q4_get_greedy_screen", "q4_screen_candidates", "q4_greedy_screen_op")
_BASE = {}


def _base(n):
    """the rows of the GPU test's shapes behave alike: 2125 of them (a ragged 64 rows x 32 blocks + 77) keep this quick"""
    if n not in _BASE:
        w = ref.base_matrix(n, 64 * 32 + 77, SEED + n)
        _BASE[n] = (w, ref.quantise(w))
    return _BASE[n]


@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("n", [4096, 5120])
def test_restated_bound_holds_against_float64(n, name):
    base, qbase = _base(n)
    w, x, g = ref.make_case(name, base, n, SEED + n)
    quant = qbase if w is None else ref.quantise(w)
    w = base if w is None else w
    xs = x if g is None else ref.rmsnorm16(x, g)
    A, B = ref.screen(*quant, xs)
    t = ref.logits64(w, xs)
    with np.errstate(over="ignore", invalid="ignore"):
        L = t.astype(np.float16).astype(np.float64)             # the exact sum rounded once: an fp32 sum of 28 roundings lies inside gamma's share of B
    claim = np.isfinite(B)
    assert np.isfinite(L[claim]).all()
    err = np.abs(A[claim] - L[claim])
    assert (err <= B[claim]).all(), "%s: worst |A - L| / B = %g" % (name, (err / B[claim]).max())
    # what the quantisation alone may cost: Cauchy-Schwarz
    q, s, E, W = quant
    X = np.sqrt((xs.astype(np.float64) ** 2).sum())
    if np.isfinite(X):
        ok = np.isfinite(E)
        assert (np.abs(A[ok] - t[ok]) <= E[ok] * X * (1 + 1e-12) + 1e-300).all()
    if name in ref.BENIGN:
        G = (A - B)[claim].max()
        assert ((A + B >= G) | ~claim).sum() <= 0.02 * w.shape[0]
    if name in ("x containing a NaN",):
        assert not claim.any()


def test_quantiser_edge_rows():
    w = np.zeros((4, 4096), dtype=np.float16)
    w[1] = 0.5
    w[2, 7] = np.inf
    w[3, ::2] = -3.0
    q, s, E, W = ref.quantise(w)
    assert s[0] == 0 and not q[0].any() and E[0] == 0 and W[0] == 0
    assert (q[1] == 127).all() and E[1] < 1e-4 and abs(W[1] - 32.0) < 1e-3
    assert s[2] == 0 and not q[2].any() and E[2] == np.inf
    assert set(q[3].tolist()) == {0, -127}


def _declared():
    src = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(q4_[A-Za-z0-9_]*)\s*\(", src))


def test_header_export_map_and_api_agree_on_the_new_symbols():
    from llama_cu_awq_amd import api
    declared = _declared()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in api.SYMBOLS, name
    assert "run_transformer_steps_screenable" not in exported      # the token loops' entry stays inside the library
    L = api.lib()
    assert L.q4_get_greedy_screen() == 1                          # on by default
    assert L.q4_screen_candidates(None, None, None, None, None) == 5   # Q4_ERR_ARG
