"""Vocoder training examples from wav files: datasets/moon.py:79-147 (`_process_utterance`, input_type 'raw'), batched over utterances.

    python -m twvk_amd.preprocess --in_dir wavs/ --out_dir data/moon        # one <name>.npz per <name>.wav

Files are read at their own rate; those not at hparams.sample_rate are resampled on the GPU first (read_chunk, audio.resample: what
librosa.load(path, sr) does in utils/audio.py:11-12), a chunk's files of one rate in one pass.
Per utterance: rescale (moon.py:80-81), trim leading / trailing silence (:84-85, utils/audio.py:46-52), mel and linear spectrogram
(:113,120 -- both from one FFT pass on the GPU, audio.spectrograms), the length rule (:116-117), and the audio reflect-padded by
fft_size // 2 and cut to mel_frames * hop_size (:135-147) so that audio and mel stay in step for the transposed-convolution
upsampling.  Each npz holds `audio`, `mel` (frames, num_mels), `linear` (frames, num_freq), `time_steps`, `mel_frames`: the keys
DataFeederWavenet (train_vocoder.py) and the reference's feeders read.  `text` / `tokens` belong to the Korean text frontend (SURVEY.md
section 2 row 17, out of scope).  Everything but the spectrograms is index logic on the host."""
import argparse
import os
from glob import glob

import numpy as np

from .hparams import default_hparams, load_hparams


def read_wav(path, sample_rate):
    """scipy.io.wavfile -> float32 in [-1, 1), channels averaged.  The reference's librosa.load(path, sr) would resample a file of
    another rate (resampy); that kernel is not restated here, so such a file is an error."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if sr != sample_rate:
        raise ValueError("%s: sample rate %d, hparams.sample_rate is %d (resampling is not built)" % (path, sr, sample_rate))
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype in (np.float32, np.float64):
        x = data.astype(np.float32)
    else:
        raise ValueError("%s: unsupported sample format %s (int16, int32 and float32 are read)" % (path, data.dtype))
    return x.mean(axis=1) if x.ndim == 2 else x


def trim_indices(wav, top_db, frame_length, hop_length):
    """librosa.effects.trim's interval [RECALLED-LIBROSA <= 0.7], float64 numpy: frame mean squares with centre / reflect padding,
    10 log10(max(1e-10, mse)) - 10 log10(max(1e-10, max mse)) > -top_db; start = first such frame * hop,
    end = min(len, (last + 1) * hop); (0, 0) when no frame passes."""
    y = np.asarray(wav, np.float64)
    yp = np.pad(y, frame_length // 2, mode="reflect")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    csum = np.concatenate([[0.0], np.cumsum(yp * yp)])
    starts = np.arange(n_frames) * hop_length
    mse = (csum[starts + frame_length] - csum[starts]) / frame_length
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(max(1e-10, mse.max()))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(nz[0] * hop_length), int(min(len(y), (nz[-1] + 1) * hop_length))


def trim_silence(wav, hparams):
    """utils/audio.py:46-52"""
    start, end = trim_indices(wav, hparams.trim_top_db, hparams.trim_fft_size, hparams.trim_hop_size)
    return wav[start:end]


def prepare_wav(wav, hparams):
    """moon.py:79-85: what the spectrograms are taken of"""
    if hparams.input_type != "raw":
        raise NotImplementedError("input_type %r: only 'raw' is built (the reference's own mulaw branches call undefined names, "
                                  "datasets/moon.py:90,97)" % (hparams.input_type,))
    wav = np.asarray(wav, np.float32)
    if hparams.rescaling:
        wav = wav / np.abs(wav).max() * hparams.rescaling_max
    if hparams.trim_silence:
        wav = trim_silence(wav, hparams)
    return wav.astype(np.float32)


def assemble_example(wav, mel, linear, hparams):
    """moon.py:113-147 after the spectrograms (host only): wav = prepare_wav's output, mel (frames, num_mels), linear (frames, num_freq).
    None where the reference skips the utterance (:116-117)."""
    if getattr(hparams, "use_lws", False):
        raise NotImplementedError("use_lws=True (hparams.py:15 default False) is not built")
    mel = np.asarray(mel, np.float32)
    linear = np.asarray(linear, np.float32)
    mel_frames = mel.shape[0]
    if mel_frames > hparams.max_mel_frames and hparams.clip_mels_length:
        return None
    assert linear.shape[0] == mel_frames
    out = np.pad(np.asarray(wav, np.float32), hparams.fft_size // 2, mode="reflect")        # librosa_pad_lr, utils/audio.py:171-174
    assert len(out) >= mel_frames * hparams.hop_size
    out = out[:mel_frames * hparams.hop_size]
    return {"audio": out.astype(np.float32), "mel": mel, "linear": linear, "time_steps": len(out), "mel_frames": mel_frames}


def process_batch(wavs, hparams, device="cuda:0"):
    """a list of raw utterances -> a list of examples (None = skipped), the spectrograms of the whole list in one device pass"""
    from .audio import spectrograms
    prepared = [prepare_wav(w, hparams) for w in wavs]
    keep = [i for i, w in enumerate(prepared) if len(w) > hparams.fft_size // 2]           # one reflection only (twv_spectrogram_analyze)
    out = [None] * len(wavs)
    if not keep:
        return out
    mel, lin = spectrograms([prepared[i] for i in keep], hparams, device=device)
    mel, lin = mel.cpu().numpy(), lin.cpu().numpy()
    for row, i in enumerate(keep):
        frames = 1 + len(prepared[i]) // hparams.hop_size
        out[i] = assemble_example(prepared[i], mel[row, :frames].copy(), lin[row, :frames].copy(), hparams)
    return out


def read_chunk(paths, sample_rate, device="cuda:0"):
    """the utterances of `paths` at `sample_rate`: a file already at that rate goes through read_wav; the others are read at their
    own rate and resampled on the GPU (audio.resample), the files that share a rate and a sample layout in one device pass"""
    from scipy.io import wavfile
    from .audio import resample, wav_samples
    out, groups = [None] * len(paths), {}
    for i, p in enumerate(paths):
        sr, data = wavfile.read(p, mmap=True)
        if sr == sample_rate:
            out[i] = read_wav(p, sample_rate)
            continue
        try:
            x = wav_samples(np.asarray(data))
        except ValueError as e:
            raise ValueError("%s: %s" % (p, e))
        groups.setdefault((sr, x.dtype.str, x.ndim), []).append((i, x))
    for (sr, _, _), members in groups.items():
        y, n = resample([x for _, x in members], sr, sample_rate, device=device)
        y = y.cpu().numpy()
        for row, (i, _) in enumerate(members):
            out[i] = y[row, :n[row]].copy()
    return out


def get_arguments(argv=None):
    parser = argparse.ArgumentParser(description="wav files -> npz examples for train_vocoder.py")
    parser.add_argument("--in_dir", required=True, help="directory of .wav files (one speaker)")
    parser.add_argument("--out_dir", required=True, help="directory the <name>.npz examples are written to")
    parser.add_argument("--batch_size", type=int, default=16, help="utterances per device pass")
    parser.add_argument("--hparams_dir", default=None, help="directory with a params.json (a trained model's) that overrides the default hparams")
    parser.add_argument("--device", default="cuda:0")
    return parser.parse_args(argv)


def main(argv=None, log=print):
    args = get_arguments(argv)
    hp = default_hparams()
    if args.hparams_dir:
        load_hparams(hp, args.hparams_dir)
    paths = sorted(glob(os.path.join(args.in_dir, "*.wav")))
    if not paths:
        raise ValueError("no .wav files in %s" % args.in_dir)
    os.makedirs(args.out_dir, exist_ok=True)
    written, skipped = [], []
    for i in range(0, len(paths), max(1, args.batch_size)):
        chunk = paths[i:i + max(1, args.batch_size)]
        examples = process_batch(read_chunk(chunk, hp.sample_rate, device=args.device), hp, device=args.device)
        for p, ex in zip(chunk, examples):
            if ex is None:
                skipped.append(p)
                log("skipped %s (more than max_mel_frames = %d frames, or shorter than fft_size / 2 after trimming)" % (p, hp.max_mel_frames))
                continue
            dst = os.path.join(args.out_dir, os.path.splitext(os.path.basename(p))[0] + ".npz")
            np.savez(dst, **ex)
            written.append(dst)
    log("wrote %d examples to %s (%d skipped)" % (len(written), args.out_dir, len(skipped)))
    return {"written": written, "skipped": skipped}


if __name__ == "__main__":
    main()
