"""What the Tacotron feed tests share (tests/test_tacotron_feed_cpu.py, tests/test_tacotron_feed_gpu.py, tests/test_train_tacotron_*.py):
the reference feeder's recorded batches (tests/golden/reference_tacotron_feeder.npz, made by tests/golden/make_reference_tacotron_feeder.py),
synthetic examples and directories of them."""
import functools
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tacotron_feeder.npz")
NAMES = ("inputs", "input_lengths", "loss_coeff", "mel_targets", "linear_targets", "speaker_id")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def feed_hp(**kw):
    """the hyper-parameters a feeder reads (hparams.py's defaults), as a plain namespace"""
    hp = types.SimpleNamespace(reduction_factor=5, min_iters=30, max_iters=200, min_tokens=30, initial_data_greedy=True, initial_phase_step=8000,
                               main_data_greedy_factor=0, main_data=[''], num_mels=80, num_freq=1025)
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def golden_hp():
    g = golden()
    return feed_hp(reduction_factor=int(g["reduction_factor"]), min_iters=0, max_iters=100, min_tokens=0, initial_phase_step=int(g["initial_phase_step"]),
                   num_mels=int(g["num_mels"]), num_freq=int(g["num_freq"]))


def write_golden_directories(root):
    """the golden file's examples as .npz files under root/speaker_<k>/: the path_dict the reference's stand-in was given"""
    g = golden()
    path_dict, i = {}, 0
    for k, count in enumerate(g["dir_counts"]):
        d = os.path.join(str(root), "speaker_%d" % k)
        os.makedirs(d)
        path_dict[d] = []
        for _ in range(int(count)):
            kw = {key: g["example%d_%s" % (i, key)] for key in ("tokens", "mel", "linear")}
            if "example%d_loss_coeff" % i in g:
                kw["loss_coeff"] = g["example%d_loss_coeff" % i]
            assert int(g["example%d_dir" % i]) == k
            p = os.path.join(d, "%04d.npz" % i)
            np.savez(p, **kw)
            path_dict[d].append(p)
            i += 1
    return path_dict


def example(rng, n_tokens, n_frames, num_mels, num_freq, speaker_id=0, loss_coeff=1.0):
    return {"tokens": rng.randint(1, 80, n_tokens).astype(np.int32), "mel": rng.uniform(-4, 4, (n_frames, num_mels)).astype(np.float32),
            "linear": rng.uniform(-4, 4, (n_frames, num_freq)).astype(np.float32), "loss_coeff": float(loss_coeff), "speaker_id": int(speaker_id),
            "name": "synthetic"}


def write_directories(root, hp, speakers=2, per_speaker=12, seed=0, frames=(6, 30), tokens=(3, 12)):
    """`speakers` directories of `per_speaker` synthetic examples of hp's num_mels / num_freq: the data_paths of a run"""
    rng = np.random.RandomState(seed)
    dirs = []
    for s in range(speakers):
        d = os.path.join(str(root), "speaker_%d" % s)
        os.makedirs(d)
        dirs.append(d)
        for i in range(per_speaker):
            ex = example(rng, int(rng.randint(tokens[0], tokens[1] + 1)), int(rng.randint(frames[0], frames[1] + 1)), hp.num_mels, hp.num_freq)
            kw = {k: ex[k] for k in ("tokens", "mel", "linear")}
            if i % 4 == 1:
                kw["loss_coeff"] = np.float32(0.75)
            np.savez(os.path.join(d, "%02d.%04d.npz" % (s, i)), **kw)
    return dirs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
