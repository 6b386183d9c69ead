"""Offline format pipeline: own weight_packer vs the reference's (bytes, padding nibbles masked) and
the converter counterpart vs the reference convert_awq_to_bin.py (sha256 manifest)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import packer_util
from conftest import GOLDEN, ROOT

PACKER = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "weight_packer")


@pytest.mark.parametrize("fmt", [1, 0])
def test_own_packer_matches_reference_golden(tmp_path, fmt):
    g = json.load(open(os.path.join(GOLDEN, "packer_goldens.json")))["old_format_%d" % fmt]
    cfg = packer_util.write_awq_dump(str(tmp_path), old_format=bool(fmt), seed=99)
    dst = str(tmp_path / "out.bin")
    subprocess.check_call([PACKER, str(tmp_path / "config.json"), str(tmp_path / "dump"), dst, str(fmt)], stdout=subprocess.DEVNULL)
    data = open(dst, "rb").read()
    assert len(data) == g["bytes"] == 362528
    assert hashlib.sha256(packer_util.mask_zero_padding(data, cfg)).hexdigest() == g["sha256_masked"]


@pytest.mark.parametrize("fmt,seed", packer_util.GQA_CASES)
def test_own_packer_matches_reference_binary(tmp_path, fmt, seed):
    """GQA dumps: own packer vs the reference weight_packer binary's output on the same dump, stored as its size and masked sha256
    (tests/golden/packer_goldens.json, written by make_goldens.packer_goldens)."""
    g = json.load(open(os.path.join(GOLDEN, "packer_goldens.json")))["gqa_old_format_%d_seed%d" % (fmt, seed)]
    cfg = packer_util.write_awq_dump(str(tmp_path), old_format=bool(fmt), seed=seed, cfg=packer_util.CFG_GQA)
    dst = str(tmp_path / "out.bin")
    subprocess.check_call([PACKER, str(tmp_path / "config.json"), str(tmp_path / "dump"), dst, str(fmt)], stdout=subprocess.DEVNULL)
    data = open(dst, "rb").read()
    assert len(data) == g["bytes"]
    assert hashlib.sha256(packer_util.mask_zero_padding(data, cfg)).hexdigest() == g["sha256_masked"]


def test_packer_output_loads(tmp_path, orc):
    """The packed file is a valid checkpoint for the loader (header + exact size)."""
    packer_util.write_awq_dump(str(tmp_path), old_format=True, seed=1)
    dst = str(tmp_path / "out.bin")
    subprocess.check_call([PACKER, str(tmp_path / "config.json"), str(tmp_path / "dump"), dst, "1"], stdout=subprocess.DEVNULL)
    m = orc.Model(dst)
    assert (m.cfg.dim, m.cfg.hidden_dim, m.cfg.n_layers, m.cfg.n_heads, m.cfg.n_kv_heads, m.cfg.vocab_size, m.cfg.seq_len) == (256, 384, 1, 2, 2, 64, 32)
    m.close()


def test_converter_matches_reference_manifest(tmp_path):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_awq_to_bin
    g = json.load(open(os.path.join(GOLDEN, "convert_goldens.json")))
    pt = str(tmp_path / "sd.pt")
    torch.save(packer_util.synthetic_state_dict(seed=4), pt)
    convert_awq_to_bin.convert(pt, str(tmp_path / "out"))
    got = {fn: hashlib.sha256(open(str(tmp_path / "out" / fn), "rb").read()).hexdigest() for fn in sorted(os.listdir(str(tmp_path / "out")))}
    assert got == g and len(got) == 28
