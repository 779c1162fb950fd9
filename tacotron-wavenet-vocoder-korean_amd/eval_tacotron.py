"""Evaluation of a Tacotron checkpoint on held-out examples: the reference's `test_model` (train_tacotron.py:154-155 -- the graph
built with mel / linear targets and rnn_decoder_test_mode=True, whose losses the training loop reports), and the teacher-forced
("ground-truth aligned") mels a vocoder is fine-tuned on.

    python -m twvk_amd.eval_tacotron --load_path LOGDIR --data_paths D1,D2 [--batch_size N] [--teacher_forced] [--mel_out_dir DIR]

Every directory of --data_paths holds the reference's Tacotron examples: `*.npz` with `tokens`, `mel`, `linear` and an optional
`loss_coeff` (datafeeder_tacotron.py:244-266); the speaker id is the directory's index.  Batches are padded as `_prepare_batch` does
(datafeeder_tacotron.py:269-300).  The four losses of tacotron.py:258-282 are printed per batch and as their mean over the batches.
With --mel_out_dir every example's output mel, cut to the example's own frame count, is written as `<speaker id>-<example name>.npy`
(frames, num_mels) float32: what synthesizer.py writes and generate.py --mel reads.

Both passes run the layers in inference mode (no dropout, moving-average batch norm); the reference's training-mode layers are not built."""
import argparse
import os
from glob import glob

import numpy as np


def str2bool(v):
    return str(v).lower() in ('true', '1')


def _round_up(x, multiple):
    rem = x % multiple
    return x if rem == 0 else x + multiple - rem


def load_example(path, speaker_id):
    """datafeeder_tacotron.py:244-266: one `.npz` -> dict(tokens, mel, linear, loss_coeff, speaker_id, name)"""
    data = np.load(path)
    return {"tokens": np.asarray(data["tokens"], np.int32), "mel": np.asarray(data["mel"], np.float32),
            "linear": np.asarray(data["linear"], np.float32),
            "loss_coeff": float(data["loss_coeff"]) if "loss_coeff" in data else 1.0,
            "speaker_id": int(speaker_id), "name": os.path.splitext(os.path.basename(path))[0]}


def fits(n_frames, max_iters, r):
    """an example can be decoded when its frames fit max_iters steps of r frames (the reference's path filter drops longer ones)"""
    return 1 <= n_frames <= max_iters * r


def split_fitting(examples, max_iters, r, log=print):
    """(kept, skipped): examples longer than max_iters * r frames are skipped with a message"""
    kept, skipped = [], []
    for ex in examples:
        n = len(ex["linear"])
        if fits(n, max_iters, r):
            kept.append(ex)
        else:
            skipped.append(ex)
            log(" [!] skipped %s: %d frames, max_iters * reduction_factor = %d" % (ex.get("name", "?"), n, max_iters * r))
    return kept, skipped


def prepare_batch(examples, r):
    """datafeeder_tacotron.py:269-300 `_prepare_batch` for evaluation (no shuffle): inputs padded with 0 to the longest, mel / linear
    targets padded with 0 to the longest frame count rounded up to a multiple of r.  (The reference rounds max + 1 up, which always leaves
    a padding frame; here the longest example may fill the last step, so that an example of exactly max_iters * r frames still decodes.)
    Returns a dict of numpy arrays: inputs (N, T_in) int32, input_lengths (N), loss_coeff (N) float32, mel_targets (N, T_out, num_mels),
    linear_targets (N, T_out, num_freq), speaker_id (N) int32, n_frames (N): each example's own frame count."""
    t_in = max(len(ex["tokens"]) for ex in examples)
    n_frames = np.asarray([len(ex["linear"]) for ex in examples], np.int32)
    t_out = _round_up(int(n_frames.max()), r)

    def pad_target(t):
        return np.pad(np.asarray(t, np.float32), [(0, t_out - len(t)), (0, 0)], mode='constant')
    return {"inputs": np.stack([np.pad(np.asarray(ex["tokens"], np.int32), (0, t_in - len(ex["tokens"])), mode='constant') for ex in examples]),
            "input_lengths": np.asarray([len(ex["tokens"]) for ex in examples], np.int32),
            "loss_coeff": np.asarray([ex.get("loss_coeff", 1.0) for ex in examples], np.float32),
            "mel_targets": np.stack([pad_target(ex["mel"]) for ex in examples]),
            "linear_targets": np.stack([pad_target(ex["linear"]) for ex in examples]),
            "speaker_id": np.asarray([ex.get("speaker_id", 0) for ex in examples], np.int32),
            "n_frames": n_frames}


LOSS_NAMES = ("loss", "mel_loss", "linear_loss", "loss_without_coeff")


def evaluate(model, examples, r, batch_size=32, teacher_forced=False, mel_out_dir=None, log=print):
    """runs `examples` through model.forward_targets / add_loss in batches; returns (per-batch list of loss dicts, their mean)"""
    per_batch = []
    if mel_out_dir:
        os.makedirs(mel_out_dir, exist_ok=True)
    for i0 in range(0, len(examples), batch_size):
        chunk = examples[i0:i0 + batch_size]
        b = prepare_batch(chunk, r)
        mel, _, _ = model.forward_targets(b["inputs"], b["input_lengths"], b["speaker_id"], b["mel_targets"], teacher_forced=teacher_forced,
                                          want_linear=True, want_alignments=False)
        losses = model.add_loss(b["linear_targets"], b["loss_coeff"])
        per_batch.append(losses)
        log("batch %d (%d examples, %d frames): " % (len(per_batch) - 1, len(chunk), b["mel_targets"].shape[1])
            + " ".join("%s=%.5f" % (k, losses[k]) for k in LOSS_NAMES))
        if mel_out_dir:
            mel = mel.cpu().numpy()
            for ex, m, n in zip(chunk, mel, b["n_frames"]):
                np.save(os.path.join(mel_out_dir, "%d-%s.npy" % (ex["speaker_id"], ex["name"])), m[:n], allow_pickle=False)
    mean = {k: float(np.mean([l[k] for l in per_batch])) for k in LOSS_NAMES} if per_batch else {}
    if per_batch:
        log("mean over %d batches: " % len(per_batch) + " ".join("%s=%.5f" % (k, mean[k]) for k in LOSS_NAMES))
    return per_batch, mean


def build_parser():
    parser = argparse.ArgumentParser(description="losses of a Tacotron checkpoint on held-out examples; ground-truth-aligned mels")
    parser.add_argument('--load_path', required=True, help='logdir of the checkpoint (model.ckpt-N + params.json) or a bundle prefix')
    parser.add_argument('--data_paths', required=True, help='comma-separated example directories; the speaker id is the index')
    parser.add_argument('--batch_size', default=32, type=int)
    parser.add_argument('--checkpoint_step', default=None, type=int)
    parser.add_argument('--teacher_forced', action='store_true', help='feed the ground-truth frames (default: free-running, the test_model)')
    parser.add_argument('--mel_out_dir', default=None, help='write every example\'s output mel, cut to its own length, as .npy')
    return parser


def main(argv=None):
    config = build_parser().parse_args(argv)
    if config.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    from .synthesizer import Synthesizer
    data_dirs = [d for d in config.data_paths.split(",") if d]
    syn = Synthesizer()
    syn.load(config.load_path, num_speakers=len(data_dirs), checkpoint_step=config.checkpoint_step)
    hp = syn.hparams
    examples = []
    for spk, d in enumerate(data_dirs):
        paths = sorted(glob(os.path.join(d, "*.npz")))
        if not paths:
            raise SystemExit("no *.npz examples in %s" % d)
        examples += [load_example(p, spk) for p in paths]
    examples, _ = split_fitting(examples, hp.max_iters, hp.reduction_factor)
    if not examples:
        raise SystemExit("no example fits max_iters * reduction_factor = %d frames" % (hp.max_iters * hp.reduction_factor))
    return evaluate(syn.model, examples, hp.reduction_factor, batch_size=config.batch_size, teacher_forced=config.teacher_forced,
                    mel_out_dir=config.mel_out_dir)[1]


if __name__ == "__main__":
    main()
