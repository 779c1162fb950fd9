"""synthesizer.py of the reference (synthesizer.py:29-388) on the MI355X path: same class, method signatures, output files and
CLI flags; `sess.run` of the Tacotron graph is ONE twv_tacotron_infer call and `inv_linear_spectrogram` (utils/audio.py:77-92,
Griffin-Lim) runs on the GPU.

    synthesizer = Synthesizer()
    synthesizer.load(load_path, num_speakers, checkpoint_step)                       # synthesizer.py:34-70
    synthesizer.synthesize(texts=[text], base_path=sample_path, speaker_ids=[0], attention_trim=True)   # :72-199
    synthesizer.synthesize_manual(tokens=..., base_path=sample_path, manual_attention_mode=1)           # :136-148, :165-198

Per utterance `plot_graph_and_save_audio` (synthesizer.py:202-287) trims the spectrograms by the attention rule, inverts the
linear spectrogram and writes `<base_path>/<time>.wav` plus the mel hand-off file `<...>.npy` that generate.py --mel reads
(synthesizer.py:279-280 -> generate.py:151); without base_path / paths it returns the wav bytes.

Out of scope here, as in SURVEY.md section 8 (they raise instead of silently doing something else): the text frontend
(`texts` need a `text_to_sequence` callable -- jamo / g2p are not part of the hot path; pass `tokens`), the alignment plots
(.png), short_concat (dead in the reference), librosa_trim.  The manual-attention feeds (`manual_alignments`, the three edits of a pass's
own alignments, `base_alignment_path`) are `Synthesizer.synthesize_manual`; `synthesize` itself still refuses those two arguments."""
import argparse
import io
import os
from datetime import datetime
from glob import glob

import numpy as np

from .hparams import hparams, load_hparams


def get_time():
    return datetime.now().strftime("%Y-%m-%d_%H-%M-%S")


def add_postfix(path, postfix):
    base, ext = path.rsplit('.', 1)
    return "{}.{}.{}".format(base, postfix, ext)


def str2bool(v):
    return str(v).lower() in ('true', '1')


def get_most_recent_checkpoint(checkpoint_dir, checkpoint_step=None):
    """synthesizer.py:289-299: the bundle prefix `model.ckpt-<N>` of a directory -- the step asked for, else the largest N that has
    a data shard on disk"""
    step = checkpoint_step
    if step is None:
        steps = []
        for shard in glob(os.path.join(checkpoint_dir, "*.ckpt-*.data-*")):
            tail = os.path.basename(shard).split(".ckpt-", 1)[1]           # "<N>.data-00000-of-00001"
            steps.append(int(tail.split(".", 1)[0]))
        if not steps:
            raise FileNotFoundError("no model.ckpt-* bundle in %s" % checkpoint_dir)
        step = max(steps)
    prefix = os.path.join(checkpoint_dir, "model.ckpt-%d" % int(step))
    print(" [*] Found latest checkpoint: %s" % prefix)
    return prefix


def _prepare_inputs(inputs):
    """datafeeder_tacotron.py:288-290: right-pad the token sequences with 0 to the longest"""
    max_len = max(len(x) for x in inputs)
    return np.stack([np.pad(np.asarray(x, np.int32), (0, max_len - len(x)), mode='constant') for x in inputs])


class Synthesizer(object):
    text_to_sequence = None        # optional callable str -> list of token ids (the reference's text frontend is not rebuilt)

    def close(self):
        self.model = None

    def load(self, checkpoint_path, num_speakers=2, checkpoint_step=None, model_name='tacotron', hparams=None, device="cuda:0"):
        """synthesizer.py:34-70.  checkpoint_path: a logdir (most recent `model.ckpt-N`, or checkpoint_step) or one bundle prefix,
        restored by variable name; also a dict / .npz of numpy arrays keyed by the same variable names (tests, tools)."""
        from .tacotron import Tacotron
        from .hparams import hparams as default_hp
        self.num_speakers = num_speakers
        hp = hparams or default_hp
        if isinstance(checkpoint_path, str) and not checkpoint_path.endswith(".npz"):
            if os.path.isdir(checkpoint_path):
                load_path = checkpoint_path
                checkpoint_path = get_most_recent_checkpoint(checkpoint_path, checkpoint_step)
            else:
                load_path = os.path.dirname(checkpoint_path)
            if os.path.exists(os.path.join(load_path, "params.json")):
                load_hparams(hp, load_path)
        print('Constructing model: %s' % model_name)
        self.hparams = hp
        self.model = Tacotron(hp, num_speakers, device=device)
        if isinstance(checkpoint_path, str) and not checkpoint_path.endswith(".npz"):
            from . import checkpoint as ckpt
            print('Loading checkpoint: %s' % checkpoint_path)
            # by variable name (synthesizer.py:69-70 Saver.restore); names TensorFlow auto-generated (dense_N, ...) may be shifted in a
            # checkpoint written by a differently-built graph: checkpoint.restore_variables falls back to (scope, shape, creation order)
            tensors = ckpt.tacotron_tensors(ckpt.restore_variables(ckpt.resolve(checkpoint_path), ckpt.tacotron_variable_specs(self.model.specs), verify=True),
                                            self.model.specs)
        else:
            tensors = dict(np.load(checkpoint_path)) if isinstance(checkpoint_path, str) else checkpoint_path
        self.model.load_weights(tensors)

    # ---- one sess.run(fetches) of synthesizer.py:160 ----
    def infer(self, tokens, speaker_ids=None, want_linear=True, manual_alignments=None):
        """manual_alignments=None: the mechanism's own pass.  Else one (T_in_i, steps) array per utterance, as `save_alignment` writes them
        (synthesizer.py:143-148): rows are padded with zeros to the batch's T_in, all must share `steps`, and the decoder attends with them
        for `steps` steps (Tacotron.infer_manual)."""
        seqs = [np.asarray(s, np.int32) for s in tokens]
        sequences = _prepare_inputs(seqs)
        input_lengths = [int(np.argmax(a == 1)) + 1 for a in sequences]                  # synthesizer.py:126
        if speaker_ids is None:
            speaker_ids = np.zeros(len(seqs), np.int32)                                  # synthesizer.py:49-50 default
        if manual_alignments is None:
            mel, lin, al = self.model.infer(sequences, input_lengths, speaker_ids, want_linear=want_linear)
        else:
            T = sequences.shape[1]
            arrays = [np.asarray(a, np.float32) for a in manual_alignments]
            if len(arrays) != len(seqs) or any(a.ndim != 2 or a.shape[0] > T or a.shape[1] != arrays[0].shape[1] for a in arrays):
                raise ValueError("manual_alignments: one (T_in <= %d, steps) array per utterance (%d), all of the same steps; got %s"
                                 % (T, len(seqs), [a.shape for a in arrays]))
            stacked = np.stack([np.pad(a, ((0, T - a.shape[0]), (0, 0)), mode='constant') for a in arrays])
            mel, lin, al = self.model.infer_manual(sequences, input_lengths, speaker_ids, self.model.edit_alignments(stacked, 0),   # synthesizer.py:147
                                                   want_linear=want_linear)
        return {"mel": mel, "linear": lin, "alignments": al, "input_lengths": input_lengths, "sequences": sequences}

    def synthesize(self, texts=None, tokens=None, base_path=None, paths=None, speaker_ids=None, start_of_sentence=None,
                   end_of_sentence=True, pre_word_num=0, post_word_num=0, pre_surplus_idx=0, post_surplus_idx=1,
                   use_short_concat=False, manual_attention_mode=0, base_alignment_path=None, librosa_trim=False,
                   attention_trim=True, isKorean=True, seed=None, griffin_lim="per_utterance"):
        """synthesizer.py:72-199.  Returns one result per utterance: True when files were written, else the wav bytes.
        griffin_lim="per_utterance" (the default) runs Griffin-Lim on one trimmed utterance after the other, as synthesizer.py:258
        does; "batched" trims them all, runs ONE audio.inv_linear_spectrogram_list call over the utterances of unequal lengths and
        writes the same files / returns the same kind of bytes per utterance (with `seed`, utterance i still draws
        RandomState(seed).rand(1, T_i, F): the stream restarts per utterance as in the loop)."""
        if griffin_lim not in ("per_utterance", "batched"):
            raise ValueError("griffin_lim must be 'per_utterance' or 'batched', got %r" % (griffin_lim,))
        if manual_attention_mode or base_alignment_path is not None:
            raise ValueError("synthesize() runs the mechanism's own pass only: manual attention (synthesizer.py:137-196) is Synthesizer.synthesize_manual")
        if use_short_concat or librosa_trim:
            raise ValueError("short_concat / librosa_trim (host DSP on text-frontend data) are out of scope of this path")
        if type(texts) == str:
            texts = [texts]
        if texts is not None and tokens is None:
            if self.text_to_sequence is None:
                raise ValueError("texts need Synthesizer.text_to_sequence (the reference's text frontend is not part of this path); "
                                 "pass tokens=[[ids..., 1], ...]")
            tokens = [self.text_to_sequence(text) for text in texts]
        if tokens is None:
            raise ValueError("texts or tokens required")
        out = self.infer(tokens, speaker_ids, want_linear=True)
        return self._save_pass(out, texts, paths, base_path, get_time(), False, start_of_sentence, end_of_sentence, attention_trim, isKorean,
                               seed, griffin_lim)

    def _save_pass(self, out, texts, paths, base_path, time_str, use_manual_attention, start_of_sentence, end_of_sentence, attention_trim,
                   isKorean, seed, griffin_lim):
        """plot_and_save_parallel (synthesizer.py:104-123) on one pass's outputs: one result per utterance"""
        sequences = out["sequences"]
        if paths is None:
            paths = [None] * len(sequences)
        if texts is None:
            texts = [None] * len(sequences)
        wavs = out["linear"].cpu().numpy()
        alignments = out["alignments"].cpu().numpy()
        mels = out["mel"].cpu().numpy()
        if griffin_lim == "batched":
            return save_audio_batched(list(enumerate(zip(wavs, alignments, paths, texts, sequences, mels))), base_path=base_path,
                                      end_of_sentence=end_of_sentence, attention_trim=attention_trim, time_str=time_str,
                                      hparams=self.hparams, seed=seed, use_manual_attention=use_manual_attention)
        results = []
        for item in enumerate(zip(wavs, alignments, paths, texts, sequences, mels)):
            results.append(plot_graph_and_save_audio(item, base_path=base_path, start_of_sentence=start_of_sentence,
                                                     end_of_sentence=end_of_sentence, use_manual_attention=use_manual_attention,
                                                     attention_trim=attention_trim, time_str=time_str,
                                                     isKorean=isKorean, hparams=self.hparams, seed=seed))
        return results

    def synthesize_manual(self, texts=None, tokens=None, base_path=None, paths=None, speaker_ids=None, manual_attention_mode=0,
                          base_alignment_path=None, manual_alignments=None, attention_trim=True, end_of_sentence=True, seed=None,
                          griffin_lim="per_utterance"):
        """The manual-attention half of synthesizer.py:72-199.

        manual_attention_mode 1, 2 or 3 (:165-198) is the reference's two passes: the plain pass, whose results are written as `synthesize`
        writes them; then its alignments edited on the device (Tacotron.edit_alignments: 1 argmax one-hot, 2 squared, 3 argmax set to 1 --
        they never visit the host) and fed back, that pass's results written with the `.manual` postfix.  Returns (results, manual_results).
        (The reference's second `sess.run` unpacks three fetches into two names and calls plot_and_save_parallel without mels, :197-198, so
        it never got this far; the graph feeds and the edit rules are what is built.)

        With mode 0 and `base_alignment_path` (:136-148) or `manual_alignments` it is ONE pass that attends with the given alignments, and
        one list is returned.  base_alignment_path is a prefix used as given: utterance idx reads "<prefix><idx>.npy", a (T_in, steps) array
        as `save_alignment` writes it (:265-267).  The reference joins the prefix behind basename(base_path) (:141), which names a
        directory relative to wherever the process runs; that join is not reproduced.  manual_alignments is that list of arrays itself.
        A mode 1-3 with given alignments edits the given pass's own output: pass one attends with them, pass two with their edit."""
        if griffin_lim not in ("per_utterance", "batched"):
            raise ValueError("griffin_lim must be 'per_utterance' or 'batched', got %r" % (griffin_lim,))
        if manual_attention_mode not in (0, 1, 2, 3):
            raise ValueError("manual_attention_mode must be 0, 1, 2 or 3, got %r" % (manual_attention_mode,))
        if base_alignment_path is not None and manual_alignments is not None:
            raise ValueError("give base_alignment_path or manual_alignments, not both")
        if not manual_attention_mode and base_alignment_path is None and manual_alignments is None:
            raise ValueError("nothing manual was asked for: manual_attention_mode 1-3, base_alignment_path or manual_alignments (else use synthesize)")
        if type(texts) == str:
            texts = [texts]
        if texts is not None and tokens is None:
            if self.text_to_sequence is None:
                raise ValueError("texts need Synthesizer.text_to_sequence (the reference's text frontend is not part of this path); "
                                 "pass tokens=[[ids..., 1], ...]")
            tokens = [self.text_to_sequence(text) for text in texts]
        if tokens is None:
            raise ValueError("texts or tokens required")
        if base_alignment_path is not None:
            manual_alignments = [np.load("{}{}.npy".format(base_alignment_path, idx)) for idx in range(len(tokens))]      # synthesizer.py:143-145
        time_str = get_time()

        def save(out, manual):
            return self._save_pass(out, texts, paths, base_path, time_str, manual, None, end_of_sentence, attention_trim, True, seed, griffin_lim)
        out = self.infer(tokens, speaker_ids, want_linear=True, manual_alignments=manual_alignments)
        results = save(out, False)                                                       # synthesizer.py:161
        if not manual_attention_mode:
            return results
        edited = self.model.edit_alignments(out["alignments"], manual_attention_mode)    # synthesizer.py:165-190, on the device
        mel, lin, al = self.model.infer_manual(out["sequences"], out["input_lengths"], self.model.speaker_id, edited)
        second = dict(out, mel=mel, linear=lin, alignments=al)
        return results, save(second, True)                                               # synthesizer.py:197-198


def plot_graph_and_save_audio(args, base_path=None, start_of_sentence=None, end_of_sentence=None, use_manual_attention=False,
                              save_alignment=False, attention_trim=False, time_str=None, isKorean=True, hparams=hparams, seed=None):
    """synthesizer.py:202-287 without the .png: attention trim -> Griffin-Lim (GPU) -> `<path>.wav` + the mel `<path>.npy`."""
    from .audio import inv_linear_spectrogram
    from .e2e import attention_trim_frames
    from .ops import wav_to_int16
    from scipy.io import wavfile
    idx, (wav, alignment, path, text, sequence, mel) = args
    if base_path:
        plot_path = "{}/{}.{}.png".format(base_path, time_str or get_time(), idx)     # one name per utterance of the batch
    elif path:
        plot_path = path.rsplit('.', 1)[0] + ".png"
    else:
        plot_path = None
    if use_manual_attention and plot_path:
        plot_path = add_postfix(plot_path, "manual")
    if attention_trim and end_of_sentence:
        spec_end_idx = attention_trim_frames(alignment, len(sequence), hparams.reduction_factor)     # synthesizer.py:232-256
        wav = wav[:spec_end_idx]
        mel = mel[:spec_end_idx]
    audio_out = inv_linear_spectrogram(wav[None], hparams, seed=seed)[0]          # synthesizer.py:258 inv_linear_spectrogram(wav.T)
    if save_alignment and base_path:
        np.save("{}/{}.npy".format(base_path, idx), alignment, allow_pickle=False)
    pcm = wav_to_int16(audio_out[None]).cpu().numpy().reshape(-1)                 # utils/audio.py:14-17 save_wav
    if path or base_path:
        current_path = add_postfix(path, idx) if path else plot_path.replace(".png", ".wav")
        os.makedirs(os.path.dirname(os.path.abspath(current_path)), exist_ok=True)
        wavfile.write(current_path, hparams.sample_rate, pcm)
        np.save(current_path.replace(".wav", ".npy"), mel)                         # synthesizer.py:279-280: the vocoder's --mel input
        return True
    io_out = io.BytesIO()
    wavfile.write(io_out, hparams.sample_rate, pcm)
    return io_out.getvalue()


def save_audio_batched(items, base_path=None, end_of_sentence=None, attention_trim=False, time_str=None, hparams=hparams, seed=None,
                       use_manual_attention=False):
    """plot_graph_and_save_audio for all utterances of a call with ONE Griffin-Lim call: every utterance is trimmed by its attention,
    audio.inv_linear_spectrogram_list runs them at their own lengths, then each gets its own peak normalisation (wav_to_int16) and
    the same files (`<path>.wav` + the mel `<path>.npy`) or bytes as the loop gives."""
    from .audio import inv_linear_spectrogram_list
    from .e2e import attention_trim_frames
    from .ops import wav_to_int16
    from scipy.io import wavfile
    trimmed = []
    for idx, (wav, alignment, path, text, sequence, mel) in items:
        if attention_trim and end_of_sentence:
            spec_end_idx = attention_trim_frames(alignment, len(sequence), hparams.reduction_factor)     # synthesizer.py:232-256
            wav, mel = wav[:spec_end_idx], mel[:spec_end_idx]
        trimmed.append((idx, wav, path, mel))
    uniforms = None
    if seed is not None:                                      # the loop's draw per utterance: the stream restarts at every one
        F = hparams.fft_size // 2 + 1
        uniforms = [np.random.RandomState(seed).rand(1, len(wav), F)[0] for _, wav, _, _ in trimmed]
    audio = inv_linear_spectrogram_list([wav for _, wav, _, _ in trimmed], hparams, uniforms=uniforms)
    results = []
    for (idx, wav, path, mel), audio_out in zip(trimmed, audio):
        pcm = wav_to_int16(audio_out[None]).cpu().numpy().reshape(-1)                 # utils/audio.py:14-17 save_wav, per utterance
        if path or base_path:
            current_path = add_postfix(path, idx) if path else "{}/{}.{}.wav".format(base_path, time_str or get_time(), idx)
            if use_manual_attention and not path:
                current_path = add_postfix(current_path, "manual")                        # the loop's `<time>.<idx>.manual.wav`
            os.makedirs(os.path.dirname(os.path.abspath(current_path)), exist_ok=True)
            wavfile.write(current_path, hparams.sample_rate, pcm)
            np.save(current_path.replace(".wav", ".npy"), mel)
            results.append(True)
        else:
            io_out = io.BytesIO()
            wavfile.write(io_out, hparams.sample_rate, pcm)
            results.append(io_out.getvalue())
    return results


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--load_path', required=True)
    parser.add_argument('--sample_path', default="logdir-tacotron/generate")
    parser.add_argument('--text', default=None)
    parser.add_argument('--tokens', default=None, help='comma-separated token ids ending in 1 (EOS): the text frontend is not part of this path')
    parser.add_argument('--num_speakers', default=1, type=int)
    parser.add_argument('--speaker_id', default=0, type=int)
    parser.add_argument('--checkpoint_step', default=None, type=int)
    parser.add_argument('--is_korean', default=True, type=str2bool)
    parser.add_argument('--base_alignment_path', default=None, help='prefix of saved alignments: utterance idx attends with "<prefix><idx>.npy"')
    parser.add_argument('--seed', default=None, type=int, help='seed of the Griffin-Lim initial phases (extension; the reference is unseeded)')
    config = parser.parse_args(argv)
    if config.text is None and config.tokens is None:
        parser.error("--text or --tokens required")
    os.makedirs(config.sample_path, exist_ok=True)
    synthesizer = Synthesizer()
    synthesizer.load(config.load_path, config.num_speakers, config.checkpoint_step)
    tokens = [[int(t) for t in config.tokens.split(",")]] if config.tokens else None
    texts = [config.text] if config.text else None
    if config.base_alignment_path is not None:
        # (the flags are the reference's, synthesizer.py:371-388, which has none for manual_attention_mode: the edits are reached from Python)
        return synthesizer.synthesize_manual(texts=texts, tokens=tokens, base_path=config.sample_path, speaker_ids=[config.speaker_id],
                                             base_alignment_path=config.base_alignment_path, attention_trim=True, seed=config.seed)[0]
    return synthesizer.synthesize(texts=texts, tokens=tokens, base_path=config.sample_path, speaker_ids=[config.speaker_id],
                                  attention_trim=True, isKorean=config.is_korean, seed=config.seed)[0]


if __name__ == "__main__":
    main()
