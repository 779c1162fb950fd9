#!/usr/bin/env python
"""Generates tests/golden/reference_numpy_audio.npz: what the reference's OWN numpy / scipy audio functions compute, as data.

`python tests/golden/make_reference_numpy_audio.py <reference checkout>` `ast`-parses the reference's utils/audio.py, takes the
function definitions that need nothing but numpy and scipy.signal -- preemphasis (:22-25), librosa_pad_lr (:171-174), _amp_to_db
(:201-203), _db_to_amp (:205-206), _normalize (:208-220), _denormalize (:222-234) -- compiles THOSE nodes (the module itself imports
librosa and TensorFlow and cannot be imported), runs them on seeded inputs under the reference's default audio hparams and under
every normalisation setting, and stores inputs and outputs only (float64 arrays).  No source text is stored.  Run once by hand where a
reference checkout exists; never by a test.  tests/test_audio_analysis_cpu.py compares tests/audio_analysis_ref.py against the file."""
import ast
import os
import sys
import types

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
WANTED = ("preemphasis", "librosa_pad_lr", "_amp_to_db", "_db_to_amp", "_normalize", "_denormalize")
# mode numbering of include/twv_amd.h: (allow_clipping_in_normalization, symmetric_mels)
MODES = {1: (True, True), 2: (True, False), 3: (False, True), 4: (False, False)}


def reference_functions(ref):
    path = os.path.join(ref, "utils", "audio.py")
    with open(path, encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in nodes) == sorted(WANTED), [n.name for n in nodes]
    ns = {"np": np, "signal": signal}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def main(ref):
    fn = reference_functions(ref)
    rng = np.random.RandomState(20240)
    hp = types.SimpleNamespace(min_level_db=-100, ref_level_db=20, max_abs_value=4., allow_clipping_in_normalization=True, symmetric_mels=True)
    out = {"min_level_db": np.float64(hp.min_level_db), "max_abs_value": np.float64(hp.max_abs_value), "preemphasis_k": np.float64(0.97)}
    wav = rng.uniform(-1, 1, 1201)
    out["wav"] = wav
    out["preemphasis"] = fn["preemphasis"](wav, 0.97, True)
    out["preemphasis_off"] = fn["preemphasis"](wav, 0.97, False)
    out["pad_lr"] = np.float64(fn["librosa_pad_lr"](wav, 2048, 300))
    # amplitudes from far below min_level (1e-5) to above 1, and exact zeros
    amp = np.concatenate([[0.0, 1e-12, 1e-5, 1.0], 10.0 ** rng.uniform(-9, 1.5, 200)])
    out["amp"] = amp
    out["amp_to_db"] = fn["_amp_to_db"](amp, hp)
    db = np.concatenate([[-100.0, 0.0], rng.uniform(-130, 30, 100)])
    out["db"] = db
    out["db_to_amp"] = fn["_db_to_amp"](db)
    # S beyond both clip edges (the clipping modes) and inside [min_level_db, 0] (the no-clip modes assert that)
    S_wide = np.concatenate([[-100.0, 0.0, -120.0, 20.0], rng.uniform(-140, 40, 200)])
    S_in = np.concatenate([[-100.0, 0.0], rng.uniform(-100, 0, 200)])
    D_wide = np.concatenate([[-4.0, 0.0, 4.0], rng.uniform(-6, 6, 200)])
    out["S_wide"], out["S_in"], out["D_wide"] = S_wide, S_in, D_wide
    for mode, (clip, sym) in MODES.items():
        hp.allow_clipping_in_normalization, hp.symmetric_mels = clip, sym
        out["normalize_%d" % mode] = fn["_normalize"](S_wide if clip else S_in, hp)
        out["denormalize_%d" % mode] = fn["_denormalize"](D_wide, hp)
        if not clip:
            try:
                fn["_normalize"](S_wide, hp)
                raised = 0.0
            except AssertionError:
                raised = 1.0
            out["normalize_%d_asserts_on_wide" % mode] = np.float64(raised)
    out = {k: np.asarray(v, np.float64) for k, v in out.items()}
    dst = os.path.join(HERE, "reference_numpy_audio.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
