"""The restatement (oracle.Model) of a fixed token sequence through one hostile checkpoint of tests/hostile_models.py, computed once per model and shared
by tests/test_hostile_network_gpu.py and tests/test_pass_hostile_gpu.py: the per-model restatement is the expensive part of both files. A checkpoint is
named by (geometry, trait, seed); the file at `path` only has to hold it -- both files write theirs with hostile_models.write_hostile_model."""
import numpy as np

_REF = {}
_F64_LAST = {}


def restatement(orc, path, key, seq, f64_positions):
    """(logits [T, vocab] f16, (K rows, V rows) [layers, T, kv_dim] f16 of every position of `seq`, f64 logits of the first f64_positions positions)"""
    key = (key, tuple(seq), f64_positions)
    if key not in _REF:
        m = orc.Model(path)
        logits = np.stack([m.forward(tok, pos) for pos, tok in enumerate(seq)])
        k, v = m.kv()
        kv = (k[:, :len(seq)].copy(), v[:, :len(seq)].copy())
        m.close()
        m = orc.Model(path)
        f64 = np.stack([m.forward_f64(tok, pos, cap=f64_positions) for pos, tok in enumerate(seq[:f64_positions])])
        m.close()
        _REF[key] = (logits, kv, f64)
    return _REF[key]


def f64_last(orc, path, key, seq):
    """the unrounded double forward's logits behind the last position of `seq` (every position is fed in order and kept)"""
    key = (key, tuple(seq))
    if key not in _F64_LAST:
        m = orc.Model(path)
        for pos, tok in enumerate(seq):
            out = m.forward_f64(tok, pos, cap=len(seq))
        m.close()
        _F64_LAST[key] = out
    return _F64_LAST[key]
