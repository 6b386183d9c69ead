"""Batched decoding (csrc/q4_batch.hip), the part that needs no GPU: the symbols leave the library and are declared, the Python mirror offers the calls,
and a call without a batch or a model is refused before anything touches a device. What needs a built model -- slot ranges, prompts, the shapes and
settings that are not admitted -- is in tests/test_batch_gpu.py."""
import ctypes as C
import os
import re

import numpy as np

from llama_cu_awq_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q4_batch_covers", "q4_batch_new", "q4_batch_delete", "q4_batch_open", "q4_batch_restore", "q4_batch_close", "q4_batch_step", "q4_batch_generate",
       "q4_batch_pos", "q4_batch_get_logits", "q4_batch_get_kv_row", "q4_batch_cache"]
ERR_ARG = 5


def test_symbols_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
    assert "#define Q4_BATCH_MAX_SLOTS 8" in header and api.BATCH_MAX_SLOTS == 8


def test_python_mirror_offers_the_calls():
    for name in ("open", "restore", "close", "delete", "step", "generate", "pos", "logits", "kv_row", "cache", "covers"):
        assert callable(getattr(api.Batch, name)), name


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    h = C.c_void_p()
    toks = np.asarray([1, 2, 3], dtype=np.int32)
    out = np.zeros(8, dtype=np.int32)
    n = C.c_int(7)
    assert L.q4_batch_covers(None) == 0
    # (without a model the null check answers first: the ranges of n_slots, slots and prompts need a built model and are tests/test_batch_gpu.py's)
    assert L.q4_batch_new(C.byref(h), None, 2) == ERR_ARG and not h.value
    assert L.q4_batch_new(None, None, 1) == ERR_ARG
    assert L.q4_batch_delete(None) == ERR_ARG
    assert L.q4_batch_open(None, 0, toks.ctypes.data, 3, 1) == ERR_ARG
    assert L.q4_batch_restore(None, 0, None, toks.ctypes.data, 3, 1) == ERR_ARG
    assert L.q4_batch_close(None, 0) == ERR_ARG
    assert L.q4_batch_step(None, None, out.ctypes.data) == ERR_ARG
    assert L.q4_batch_generate(None, None, 4, out.ctypes.data, C.byref(n)) == ERR_ARG and n.value == 7
    assert L.q4_batch_pos(None, 0) == -ERR_ARG
    assert L.q4_batch_get_logits(None, 0, out.ctypes.data) == ERR_ARG
    assert L.q4_batch_get_kv_row(None, 0, 0, 0, out.ctypes.data, out.ctypes.data) == ERR_ARG
    assert L.q4_batch_cache(None, 0, C.byref(h), C.byref(h)) == ERR_ARG
