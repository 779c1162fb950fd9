#!/usr/bin/env python
"""Generates tests/golden/reference_tacotron_feeder.npz: what the reference's OWN Tacotron data feeder feeds, as data.

`python tests/golden/make_reference_tacotron_feeder.py <reference checkout>` `ast`-parses the reference's datasets/datafeeder_tacotron.py
(the module imports TensorFlow and cannot be imported), takes the function definitions _prepare_batch (:269-285), _prepare_inputs,
_prepare_targets, _pad_input, _pad_target, _round_up (:288-314) and, out of the class DataFeederTacotron, the methods _get_next_example
(:228-266) and _enqueue_next_group (:194-225), compiles THOSE nodes and drives them with a stand-in `self`: a given path_dict over a small
seeded directory of synthetic examples (written to a temporary directory), integers for the placeholders and a session object that
records every feed_dict.  Four groups are run, two on each side of initial_phase_step.  Stored: the examples, every recorded batch, and
the example indices in feed order -- data only, no source text.  Run once by hand where a reference checkout exists; never by a test.
tests/test_tacotron_feed_cpu.py compares twvk_amd.tacotron_feed against the file."""
import ast
import os
import sys
import tempfile
import time
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FUNCTIONS = ("_prepare_batch", "_prepare_inputs", "_prepare_targets", "_pad_input", "_pad_target", "_round_up")
METHODS = ("_get_next_example", "_enqueue_next_group")
NUM_MELS, NUM_FREQ, R = 4, 5, 3
BATCH_SIZE, BATCHES_PER_GROUP, INITIAL_PHASE_STEP, SEED = 4, 3, 6, 7
# 36 examples.  The two groups of the initial phase take 6 + 6 from each directory (offsets 2 .. 13: no wrap-around); the two groups after
# it take 9 + 9 and 3 + 3, so speaker_a wraps around and reshuffles inside the third group and speaker_b inside the fourth
DIRS = (("speaker_a", 20), ("speaker_b", 16))
DATA_RATIO = (0.75, 0.25)                            # after the initial phase: 9 and 3 of a group's 12 examples
GROUPS = 4
NAMES = ("inputs", "input_lengths", "loss_coeff", "mel_targets", "linear_targets", "speaker_id")


def reference_functions(ref):
    path = os.path.join(ref, "datasets", "datafeeder_tacotron.py")
    with open(path, encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DataFeederTacotron"][0]
    nodes += [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in nodes) == sorted(FUNCTIONS + METHODS), [n.name for n in nodes]
    ns = {"np": np, "os": os, "time": time, "_pad": 0, "log": lambda *a, **k: None, "remove_file": lambda p: None}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def synthetic_examples():
    """per directory a list of (tokens int32, mel, linear, loss_coeff or None); mel[0, 0] of example i (counted over both directories) is
    1000 + i, which is how a fed row is recognised"""
    rng = np.random.RandomState(20250)
    out, i = [], 0
    for _, count in DIRS:
        rows = []
        for _ in range(count):
            n_frames, n_tokens = int(rng.randint(1, 13)), int(rng.randint(1, 10))
            mel = rng.uniform(-4, 4, (n_frames, NUM_MELS)).astype(np.float32)
            mel[0, 0] = 1000 + i
            rows.append((rng.randint(1, 80, n_tokens).astype(np.int32), mel, rng.uniform(-4, 4, (n_frames, NUM_FREQ)).astype(np.float32),
                         None if i % 3 else np.float32(0.5 + 0.125 * i)))
            i += 1
        out.append(rows)
    return out


class Session(object):
    def __init__(self):
        self.fed = []

    def run(self, op, feed_dict):
        self.fed.append({NAMES[k]: np.array(v) for k, v in feed_dict.items()})


def main(ref):
    fn = reference_functions(ref)
    examples = synthetic_examples()
    out = {"num_mels": NUM_MELS, "num_freq": NUM_FREQ, "reduction_factor": R, "batch_size": BATCH_SIZE, "batches_per_group": BATCHES_PER_GROUP,
           "initial_phase_step": INITIAL_PHASE_STEP, "seed": SEED, "data_ratio": np.asarray(DATA_RATIO), "groups": GROUPS,
           "dir_counts": np.asarray([c for _, c in DIRS])}
    with tempfile.TemporaryDirectory() as tmp:
        path_dict, i = {}, 0
        for (name, _), rows in zip(DIRS, examples):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            path_dict[d] = []
            for tokens, mel, linear, coeff in rows:
                p = os.path.join(d, "%04d.npz" % i)
                kw = {"tokens": tokens, "mel": mel, "linear": linear}
                if coeff is not None:
                    kw["loss_coeff"] = coeff
                np.savez(p, **kw)
                path_dict[d].append(p)
                for k, v in kw.items():
                    out["example%d_%s" % (i, k)] = v
                out["example%d_dir" % i] = len(path_dict) - 1
                i += 1
        dirs = list(path_dict)
        session = Session()
        self = types.SimpleNamespace(
            _hp=types.SimpleNamespace(reduction_factor=R, initial_data_greedy=True, initial_phase_step=INITIAL_PHASE_STEP),
            batch_size=BATCH_SIZE, static_batches=None, data_dirs=dirs, _step=0, _batches_per_group=BATCHES_PER_GROUP,
            data_ratio=dict(zip(dirs, DATA_RATIO)), rng=np.random.RandomState(SEED), data_type="train", _placeholders=list(range(6)),
            _session=session, _enqueue_op=None, path_dict=path_dict, _offset=defaultdict(lambda: 2), skip_path_filter=False,
            data_dir_to_id={d: k for k, d in enumerate(dirs)})
        self._get_next_example = lambda data_dir: fn["_get_next_example"](self, data_dir)
        offsets_before = dict(self._offset)
        assert not offsets_before
        group_sizes = []
        for _ in range(GROUPS):
            before = len(session.fed)
            fn["_enqueue_next_group"](self)
            group_sizes.append(len(session.fed) - before)
    order = []
    for b, fed in enumerate(session.fed):
        for k in NAMES:
            out["batch%d_%s" % (b, k)] = fed[k]
        ids = (fed["mel_targets"][:, 0, 0] - 1000).astype(np.int64)
        assert np.array_equal(fed["mel_targets"][:, 0, 0], 1000.0 + ids)
        order.append(ids)
    out["n_batches"], out["group_sizes"] = len(session.fed), np.asarray(group_sizes)
    out["feed_order"] = np.stack(order)                    # (batches, batch_size): example indices in feed order
    out = {k: np.asarray(v) for k, v in out.items()}
    dst = os.path.join(HERE, "reference_tacotron_feeder.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "arrays;", out["n_batches"], "batches, feed order\n", out["feed_order"])


if __name__ == "__main__":
    main(sys.argv[1])
