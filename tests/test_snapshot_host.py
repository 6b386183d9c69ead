"""Sequence snapshots without a GPU: q4_snapshot_check on blobs built by hand from the documented layout, null arguments to every new entry point,
and the new names in the header, the export map and api.SYMBOLS."""
import ctypes as C
import fnmatch
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT
from llama_cu_awq_amd import api

ERR_ARG = 5
NEW = ["q4_resume_sequence", "q4_common_prefix", "q4_generate_ids_from", "q4_snapshot_new", "q4_snapshot_restore", "q4_snapshot_delete",
       "q4_snapshot_info", "q4_snapshot_tokens", "q4_snapshot_export", "q4_snapshot_import", "q4_snapshot_check", "q4_copy_runs"]
MAGIC, VERSION, HEADER = 0x4E533451, 1, 48          # "Q4SN"


def blob(kv_format=0, n_layers=2, n_kv_heads=2, head_size=64, n_pos=5, theta=10000.0, fingerprint=0x1234567890ABCDEF, magic=MAGIC, version=VERSION,
         payload=None, rows=None):
    """The serialised form, written from include/llama2_q4.h's description: header, tokens, K rows, V rows (FP8: K exponents, V exponents)."""
    elem = 1 if kv_format == 1 else 2
    implied = 2 * n_layers * n_pos * n_kv_heads * head_size * elem + (2 * n_layers * n_kv_heads * n_pos if kv_format == 1 else 0)
    head = struct.pack("<IIiiiiifQQ", magic, version, kv_format, n_layers, n_kv_heads, head_size, n_pos, theta, fingerprint,
                       (implied if payload is None else payload) & (2**64 - 1))
    assert len(head) == HEADER
    if rows is None:          # only as many bytes as a well-formed blob of plausible size has
        rows = implied if 0 <= implied < (1 << 24) and 0 < n_pos < (1 << 16) else 64
    tokens = np.arange(max(0, min(n_pos, 1 << 16)), dtype="<i4").tobytes()
    return head + tokens + (np.arange(rows, dtype=np.uint32) * 7 % 251).astype(np.uint8).tobytes()


def check(b, want_info=True):
    info = api.SnapshotInfo()
    rc = api.lib().q4_snapshot_check(b, len(b), C.byref(info) if want_info else None)
    return rc, info


def test_a_valid_blob_passes_and_reports_its_header():
    for fmt in (0, 1):
        b = blob(kv_format=fmt)
        rc, info = check(b)
        assert rc == 0
        elem = 2 - fmt
        payload = 2 * 2 * 5 * 2 * 64 * elem + fmt * 2 * 2 * 2 * 5
        assert (info.n_pos, info.kv_format, info.n_layers, info.n_kv_heads, info.head_size) == (5, fmt, 2, 2, 64)
        assert info.rope_theta == 10000.0 and info.fingerprint == 0x1234567890ABCDEF
        assert info.device_bytes == payload and info.export_bytes == HEADER + 4 * 5 + payload == len(b)
        assert check(b, want_info=False)[0] == 0
        assert api.snapshot_check(b)["n_pos"] == 5


@pytest.mark.parametrize("what, b", [
    ("truncated by one byte", blob()[:-1]),
    ("one byte of padding", blob() + b"\0"),
    ("wrong magic", blob(magic=MAGIC ^ 1)),
    ("wrong version", blob(version=2)),
    ("n_pos zero", blob(n_pos=0)),
    ("n_pos negative", blob(n_pos=-5)),
    ("n_layers negative", blob(n_layers=-2)),
    ("n_kv_heads zero", blob(n_kv_heads=0)),
    ("head_size negative", blob(head_size=-64)),
    ("kv format unknown", blob(kv_format=2)),
    ("payload field disagrees", blob(payload=16)),
    ("rope_theta not finite", blob(theta=float("nan"))),
    # 2 * 4096 * 3 * 4096 * 64 * 2 = 2^38 + ...: past 32 bits, inside 63 -- the size is computed in 64 bits and `bytes` is not it
    ("product past 32 bits", blob(n_layers=4096, n_kv_heads=4096, head_size=64, n_pos=3)),
    # the same counts whose low 32 bits make a small, plausible size: 2 * 65536 * 1 * 65536 * 1 * 2 = 2^34 -> 0 in 32 bits
    ("product that wraps to a small value in 32 bits", blob(n_layers=65536, n_kv_heads=65536, head_size=1, n_pos=1, payload=0, rows=0)),
    # 2 * 2^31 * 2^31 * 2^31 * 2: past 63 bits (and every count past its range)
    ("product past 63 bits", blob(n_layers=2**31 - 1, n_kv_heads=2**31 - 1, head_size=2**31 - 1, n_pos=2**31 - 1, payload=0)),
    ("counts at their limits", blob(n_layers=65536, n_kv_heads=65536, head_size=65536, n_pos=128 * 1024, payload=0)),
    ("header only", blob()[:HEADER]),
    ("less than a header", blob()[:HEADER - 1]),
])
def test_a_malformed_blob_is_an_argument_error(what, b):
    assert check(b)[0] == ERR_ARG, what
    h = C.c_void_p()
    assert api.lib().q4_snapshot_import(C.byref(h), b, len(b)) == ERR_ARG, what      # import checks first: no allocation, no GPU call
    assert not h.value


def test_zero_bytes_and_null_blob():
    L = api.lib()
    assert L.q4_snapshot_check(blob(), 0, None) == ERR_ARG
    assert L.q4_snapshot_check(None, 0, None) == ERR_ARG
    assert L.q4_snapshot_check(None, 100, None) == ERR_ARG


def test_null_arguments_to_every_new_entry_point():
    L = api.lib()
    h = C.c_void_p()
    toks = np.array([1, 2, 3], dtype=np.int32)
    buf = np.zeros(64, dtype=np.uint8)
    assert L.q4_resume_sequence(None, toks.ctypes.data, 3, 1) == ERR_ARG
    assert L.q4_common_prefix(None, toks.ctypes.data, 3) == -ERR_ARG          # (a count elsewhere: the error is the one negative value)
    assert L.q4_generate_ids_from(None, None, toks.ctypes.data, 3, 8, 1, None, None, None) == -1.0   # like every failure of q4_generate_ids
    assert L.q4_snapshot_new(None, None, 1) == ERR_ARG
    assert L.q4_snapshot_new(C.byref(h), None, 1) == ERR_ARG and not h.value
    assert L.q4_snapshot_restore(None, None) == ERR_ARG
    assert L.q4_snapshot_delete(None) == ERR_ARG
    assert L.q4_snapshot_info(None, C.byref(api.SnapshotInfo())) == ERR_ARG
    assert L.q4_snapshot_tokens(None, toks.ctypes.data) == ERR_ARG
    assert L.q4_snapshot_export(None, buf.ctypes.data, 64) == ERR_ARG
    assert L.q4_snapshot_import(None, blob(), len(blob())) == ERR_ARG
    assert L.q4_snapshot_import(C.byref(h), None, 0) == ERR_ARG and not h.value
    assert L.q4_copy_runs(None, buf.ctypes.data, 1, 16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(buf.ctypes.data, None, 1, 16, 16, 16) == ERR_ARG


def test_copy_runs_refuses_bad_shapes_without_a_launch():
    """the argument checks come before anything touches the GPU: host addresses stand in for device pointers"""
    L = api.lib()
    a = np.zeros(256, dtype=np.uint8)
    b = np.zeros(256, dtype=np.uint8)
    pa, pb = a.ctypes.data, b.ctypes.data
    assert L.q4_copy_runs(pa, pb, -1, 16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(pa, pb, 2, -16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(pa, pb, 2, 16, -16, 16) == ERR_ARG
    assert L.q4_copy_runs(pa, pb, 2, 16, 16, -1) == ERR_ARG
    assert L.q4_copy_runs(pa, pb, 2, 15, 16, 16) == ERR_ARG          # run above the destination stride
    assert L.q4_copy_runs(pa, pb, 2, 16, 15, 16) == ERR_ARG          # ... above the source stride
    assert L.q4_copy_runs(pa, pa + 8, 1, 16, 16, 16) == ERR_ARG      # overlapping ranges
    assert L.q4_copy_runs(pa + 100, pa, 3, 40, 40, 30) == ERR_ARG    # the source's last run reaches into the destination's first
    assert L.q4_copy_runs(pa, pa, 1, 16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(pa, pb, 0, 16, 16, 16) == 0                # nothing to copy: no launch either
    assert L.q4_copy_runs(pa, pb, 4, 16, 16, 0) == 0


def test_new_symbols_in_the_header_the_export_map_and_the_bindings():
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", exports, flags=re.S).group(1).replace("\n", " ").split(";") if p.strip()]
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in api.SYMBOLS, name
        assert hasattr(L, name), name
    assert C.sizeof(api.SnapshotInfo) == 48
