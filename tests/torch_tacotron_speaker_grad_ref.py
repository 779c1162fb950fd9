"""The checker of the Tacotron speaker-side gradient and of the training step (twv_tacotron_speaker_grad, Tacotron.speaker_grad /
variable_gradients, TacotronTrainer): tests/torch_tacotron_cbhg_grad_ref.py `speaker_side`'s lines with the speaker tensors as autograd
leaves, the whole-model gradient with them, the reference's update rule (tacotron.py:285-313: clip_by_global_norm(1.0), Adam) in numpy
float64 and its learning-rate schedule restated.  Test infrastructure only; host only.

float64 is the checker, float32 the yardstick (tests/train_cases.py RATIO / FLOOR)."""
import numpy as np
import torch

import torch_tacotron_cbhg_grad_ref as CG
import torch_tacotron_grad_ref as G
import torch_tacotron_ref as R


def _tables(dims):
    return ["before_highway", "encoder_rnn_init_state", "attention_rnn_init_state"] + ["decoder_rnn_init_states%d" % (i + 1) for i in range(dims.dec_layers)]


def speaker_names(w, dims):
    """the speaker tensors of a multi-speaker model: the table and its 3 + dec_layers dense layers, or the tables of speaker_embedding_size 1"""
    if "speaker_embedding" not in w:
        return _tables(dims)
    return ["speaker_embedding"] + [("dense" if i == 0 else "dense_%d" % i) + part for i in range(3 + dims.dec_layers) for part in ("/kernel", "/bias")]


def _speaker_side(wt, dims, ids):
    """CG.speaker_side's lines on tensors: (before_highway, encoder_rnn_init, decoder_init)"""
    if "speaker_embedding" not in wt:
        v = [R._t(wt[t])[ids] for t in _tables(dims)]
    else:
        spk = R._t(wt["speaker_embedding"])[ids]
        softsign = lambda t: t / (t.abs() + 1.0)
        v = [R._dense(spk, wt, "dense" if i == 0 else "dense_%d" % i, softsign) for i in range(3 + dims.dec_layers)]
    return v[0], v[1], torch.cat(v[2:], dim=1)


def speaker_side(w, dims, speaker_ids, dtype=torch.float64):
    """the forward alone, numpy in `dtype` (the function central differences are taken of; CG.speaker_side's values)"""
    with G._as_dtype(dtype, CG.new_record()), torch.no_grad():
        wt = CG._leaves(w, speaker_names(w, dims), dtype, False)
        return [t.numpy() for t in _speaker_side(wt, dims, torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long))]


def speaker_vjp(w, dims, speaker_ids, d_before_highway, d_encoder_rnn_init, d_init, dtype=torch.float64):
    """the vector-Jacobian product of the speaker side with the three cotangents: {name: gradient} over speaker_names"""
    names = speaker_names(w, dims)
    with G._as_dtype(dtype, CG.new_record()):
        wt = CG._leaves(w, names, dtype, True)
        out = _speaker_side(wt, dims, torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long))
        total = sum((o * torch.as_tensor(np.asarray(c), dtype=dtype)).sum() for o, c in zip(out, (d_before_highway, d_encoder_rnn_init, d_init)))
        total.backward()
        return {k: CG._grad_of(wt[k], k) for k in names}


def variable_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff, prioritize_loss,
                 sample_rate, num_freq, dtype=torch.float64):
    """CG.loss_vjp's gradients plus speaker_vjp on its three hand-off cotangents: (loss, grads, record), grads over every trainable tensor
    of the model and the hand-off entries"""
    loss, _, _, grads, rec = CG.loss_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff,
                                         prioritize_loss, sample_rate, num_freq, dtype=dtype)
    grads = dict(grads)
    if dims.n_speakers > 1:
        grads.update(speaker_vjp(w, dims, speaker_ids, grads["d_before_highway"], grads["d_encoder_rnn_init"],
                                 grads["d_init"], dtype=dtype))
    return loss, grads, rec


def learning_rate(lr0, step, mode, randomly_initialized):
    """tacotron.py:292-303, step = global_step + 1"""
    if mode == 0:
        warmup = 4000.0 if randomly_initialized else 40000.0
        return lr0 * np.sqrt(warmup) * min(step / warmup ** 1.5, 1.0 / np.sqrt(step))
    return lr0 * np.exp(np.log(0.95) * step / 3000.0)


def train_step(variables, grads, m, v, t, lr, beta1, beta2, epsilon=1e-8, clip_norm=1.0):
    """tf.clip_by_global_norm(grads, clip_norm) then tf.train.AdamOptimizer.apply_gradients (t = 1-based update count), numpy float64.
    Dicts by name; a (4, C) batch norm variable takes a (2, C) gradient (d_gamma, d_beta), its moving statistics none.
    Returns (variables, m, v, the gradient's global norm before the clip, the clipped gradient)."""
    g = {}
    for k, var in variables.items():
        a = np.asarray(grads[k], np.float64)
        if a.shape != np.shape(var):
            a = np.concatenate([a, np.zeros((np.shape(var)[0] - a.shape[0],) + a.shape[1:])])
        g[k] = a
    norm = float(np.sqrt(sum(float((a * a).sum()) for a in g.values())))
    scale = clip_norm / max(norm, clip_norm)
    lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    nv, nm, nvv, clipped = {}, {}, {}, {}
    for k, var in variables.items():
        c = g[k] * scale
        nm[k] = beta1 * np.asarray(m[k], np.float64) + (1.0 - beta1) * c
        nvv[k] = beta2 * np.asarray(v[k], np.float64) + (1.0 - beta2) * c * c
        nv[k] = np.asarray(var, np.float64) - lr_t * nm[k] / (np.sqrt(nvv[k]) + epsilon)
        clipped[k] = c
    return nv, nm, nvv, norm, clipped
