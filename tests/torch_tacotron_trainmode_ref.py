"""The checker of the Tacotron training-mode graph (tacotron.py `is_training=True`): the CBHG and the whole-model loss of
tests/torch_tacotron_cbhg_grad_ref.py with `tf.layers.batch_normalization(training=True)` after every convolution -- the mean and the
biased variance over ALL N * T rows, padded ones included, differentiated through -- and dropout multipliers at the four prenet sites.
Test infrastructure only.

Nothing of the existing checkers is edited: inside `batch_norm_training` torch_tacotron_ref._batch_norm_inference, which their `_conv_block`
looks up at every call, is the batch form, and records each batch norm's statistics in call order (bank 1 .. K, proj_1, proj_2: the
order of Tacotron.batch_statistics).  The decoder is restated here once more because its prenet takes masks.

float64 is the checker, float32 the yardstick; the branch record (relu margins, pool gaps, branches taken) is that module's."""
import contextlib

import numpy as np
import torch

import torch_attention_ref as AR
import torch_tacotron_cbhg_grad_ref as CG
import torch_tacotron_grad_ref as G
import torch_tacotron_ref as R

GP = G.GP
MOMENTUM = 0.99          # tf.layers.batch_normalization's default; modules.py:92-96 passes none  [RECALLED-TF, unpinned]


@contextlib.contextmanager
def batch_norm_training(stats):
    """batch-statistics batch norm in place of the inference form; `stats` receives (mean, variance) of every call as numpy"""
    old = R._batch_norm_inference

    def batch_form(x, bn):
        gamma, beta = R._t(bn[0]), R._t(bn[1])
        flat = x.reshape(-1, x.shape[-1])
        mean = flat.mean(dim=0)
        var = ((flat - mean) ** 2).mean(dim=0)              # tf.nn.moments: biased
        stats.append((mean.detach().numpy().copy(), var.detach().numpy().copy()))
        # tf.nn.batch_normalization's own order of operations (nn_impl.py: inv = rsqrt(variance + epsilon) * scale; x * inv + (offset -
        # mean * inv)), which tacotron.bn_inference_vectors and the kernels follow.  In float64 it is (x - mean) * rsqrt(var + eps) * gamma +
        # beta to 1e-16; in float32 it is the reference's arithmetic, so the yardstick carries the reference's own cancellation where a
        # variance is tiny against epsilon (inv = gamma / sqrt(epsilon) = 31.6 gamma, and x * inv and mean * inv nearly cancel)
        inv = gamma / torch.sqrt(var + R.BN_EPSILON)
        return x * inv + (beta - mean * inv)
    R._batch_norm_inference = batch_form
    try:
        yield
    finally:
        R._batch_norm_inference = old


def _named_stats(stats, names):
    """the recorded statistics by the batch norms' checkpoint names (in spec order = call order), each (2, C)"""
    bns = [n for n in names if n.endswith("batch_normalization")]
    assert len(bns) == len(stats), (len(bns), len(stats))
    return {n: np.stack(s) for n, s in zip(bns, stats)}


def encoder_vjp(w, names, dims, tokens, lengths, before_highway=None, rnn_init=None, d_memory=None, masks=None, dtype=torch.float64):
    """torch_tacotron_cbhg_grad_ref.encoder_vjp in training mode: (memory, grads, record, statistics by name)"""
    stats = []
    with batch_norm_training(stats):
        memory, grads, rec = CG.encoder_vjp(w, names, dims, tokens, lengths, before_highway, rnn_init, d_memory, masks, dtype)
    return memory, grads, rec, _named_stats(stats, names)


def postnet_vjp(w, names, dims, mel, d_linear=None, dtype=torch.float64):
    """torch_tacotron_cbhg_grad_ref.postnet_vjp in training mode: (linear, grads, record, statistics by name)"""
    stats = []
    with batch_norm_training(stats):
        linear, grads, rec = CG.postnet_vjp(w, names, dims, mel, d_linear, dtype)
    return linear, grads, rec, _named_stats(stats, names)


def _decoder(wt, dims, mem, init, lengths, attention_type, mel_targets, masks, dtype):
    """torch_tacotron_cbhg_grad_ref._decoder with the prenet's two dropout multipliers: masks[i] is (N, steps, dec_prenet_sizes[i]) or masks None"""
    tg = np.asarray(mel_targets)
    N, t_out, M = tg.shape
    RR = dims.r
    steps = t_out // RR
    fed = torch.as_tensor(tg[:, RR - 1::RR, :], dtype=dtype)
    T_in = mem.shape[1]
    mask = torch.as_tensor(np.arange(T_in)[None, :] < np.asarray(lengths)[:, None])
    values = mem * mask[:, :, None].to(dtype)
    keys = values @ R._t(wt["memory_layer/kernel"])
    mech = AR._Mechanism(attention_type, wt, keys, mask)
    AS = wt["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
    DR = wt[GP + "cell_1/gru_cell/candidate/bias"].shape[0]
    att_h = init[:, :AS]
    dec_h = [init[:, AS + i * DR:AS + (i + 1) * DR] for i in range(dims.dec_layers)]
    context = torch.zeros(N, mem.shape[2], dtype=dtype)
    state = mech.initial_state(N, T_in)
    frame = torch.zeros(N, M, dtype=dtype)
    dm = None if masks is None else [torch.as_tensor(np.asarray(m), dtype=dtype) for m in masks]
    mel_steps = []
    for time in range(steps):
        p = R._dense(frame, wt, "decoder/decoder_prenet/dense_1", torch.relu)
        if dm is not None:
            p = p * dm[0][:, time]
        p = R._dense(p, wt, "decoder/decoder_prenet/dense_2", torch.relu)
        if dm is not None:
            p = p * dm[1][:, time]
        att_h = R._gru_cell(torch.cat([p, context], dim=-1), att_h, wt, "decoder/attention_wrapper/gru_cell")
        align, state = mech(att_h, state)
        context = (align[:, None, :] @ values)[:, 0]
        y = R._dense(torch.cat([att_h, context], dim=-1), wt, GP + "cell_0/output_projection_wrapper")
        for i in range(dims.dec_layers):
            dec_h[i] = R._gru_cell(y, dec_h[i], wt, GP + "cell_%d/gru_cell" % (i + 1))
            y = y + dec_h[i]
        out = R._dense(y, wt, "decoder/output_projection_wrapper")
        mel_steps.append(out.reshape(N, RR, M))
        frame = fed[:, time, :]
    return torch.cat(mel_steps, dim=1)


def loss_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff, prioritize_loss, sample_rate,
             num_freq, masks=None, dtype=torch.float64):
    """the whole model in training mode from the tokens, teacher-forced, and the gradient of add_loss's `loss`.  masks: None or the four
    dropout multipliers (encoder prenet 1, 2, decoder prenet 1, 2).  Returns (loss, mel, linear, grads, record, statistics by name); grads
    as torch_tacotron_cbhg_grad_ref.loss_vjp's."""
    names = CG.model_names(specs)
    rec = CG.new_record()
    stats = []
    N = np.asarray(tokens).shape[0]
    bh_np, ei_np, di_np = CG.speaker_side(w, dims, speaker_ids, dtype)
    with G._as_dtype(dtype, rec), batch_norm_training(stats):
        wt = CG._leaves(w, names, dtype, True)
        bh, ei = CG._leaf(bh_np, dtype, True), CG._leaf(ei_np, dtype, True)
        AS = wt["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
        DR = wt[GP + "cell_1/gru_cell/candidate/bias"].shape[0]
        di = CG._leaf(di_np if di_np is not None else np.zeros((N, AS + dims.dec_layers * DR)), dtype, True)
        memory = CG._encoder(wt, dims, tokens, lengths, bh, ei, None if masks is None else masks[:2], rec, dtype)
        mel = _decoder(wt, dims, memory, di, lengths, attention_type, mel_targets, None if masks is None else masks[2:], dtype)
        post = CG._cbhg(mel, None, wt, "post_cbhg", dims.post_bank, 2, dims.post_hw_depth, rec=rec)
        linear = R._dense(post, wt, CG.postnet_names(specs)[-2][:-len("/kernel")])
        mt, lt = torch.as_tensor(np.asarray(mel_targets), dtype=dtype), torch.as_tensor(np.asarray(linear_targets), dtype=dtype)
        a, b = CG._loss_terms(mel, linear, mt, lt, torch.as_tensor(np.asarray(loss_coeff), dtype=dtype), prioritize_loss, sample_rate, num_freq)
        loss = a + b
        with torch.no_grad():
            rec["loss_margin"] = min(float((mel - mt).abs().min()), float((linear - lt).abs().min()))
        loss.backward()
        grads = {k: CG._grad_of(wt[k], k) for k in names}
        grads["d_init"] = CG._grad_of(di)
        if bh is not None:
            grads["d_before_highway"], grads["d_encoder_rnn_init"] = CG._grad_of(bh), CG._grad_of(ei)
    return float(loss.detach()), mel.detach().numpy(), linear.detach().numpy(), grads, rec, _named_stats(stats, names)


def moving_average(moving, batch, momentum=MOMENTUM):
    """tf's assign_moving_average without zero-debias, float64: m - (m - batch) (1 - momentum).  For a rank-3 input the unfused batch norm
    is taken, so the moving variance receives the BIASED batch variance [RECALLED-TF, unpinned]"""
    m, b = np.asarray(moving, np.float64), np.asarray(batch, np.float64)
    return m - (m - b) * (1.0 - momentum)


def variable_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff, prioritize_loss,
                 sample_rate, num_freq, masks=None, dtype=torch.float64):
    """loss_vjp's gradients plus the speaker side's (torch_tacotron_speaker_grad_ref.speaker_vjp on the three hand-off cotangents; no batch
    norm and no dropout in it): (loss, grads, record, statistics)"""
    import torch_tacotron_speaker_grad_ref as SG
    loss, _, _, grads, rec, stats = loss_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff,
                                             prioritize_loss, sample_rate, num_freq, masks=masks, dtype=dtype)
    grads = dict(grads)
    if dims.n_speakers > 1:
        grads.update(SG.speaker_vjp(w, dims, speaker_ids, grads["d_before_highway"], grads["d_encoder_rnn_init"], grads["d_init"], dtype=dtype))
    return loss, grads, rec, stats


def train_steps(w, specs, dims, batch, masks_of_step, lr_of_step, beta1, beta2, steps, prioritize_loss, sample_rate, num_freq, attention_type,
                dtype=torch.float64):
    """`steps` training-mode steps of the checker on one batch = (tokens, lengths, speaker_ids, mel_targets, linear_targets, loss_coeff):
    gradients in `dtype`, then clip + Adam (torch_tacotron_speaker_grad_ref.train_step) and the moving averages in numpy float64.
    masks_of_step(k) gives step k's four masks (k from 0), lr_of_step(k + 1) its rate.  Returns (losses before each update, variables, the
    sum of |gradient| over all variables at the last step)."""
    import torch_tacotron_speaker_grad_ref as SG
    var = {k: np.asarray(v, np.float64) for k, v in w.items()}
    m = {k: np.zeros_like(v) for k, v in var.items()}
    v2 = {k: np.zeros_like(v) for k, v in var.items()}
    tok, ln, spk, tgt, lin_tgt, coeff = batch
    losses = []
    for k in range(steps):
        loss, grads, _, stats = variable_vjp(var, specs, dims, tok, ln, spk, attention_type, tgt, lin_tgt, coeff, prioritize_loss, sample_rate, num_freq,
                                             masks=masks_of_step(k), dtype=dtype)
        losses.append(loss)
        g1 = float(sum(np.abs(np.asarray(grads[n], np.float64)).sum() for n in var))
        var, m, v2, _, _ = SG.train_step(var, {n: grads[n] for n in var}, m, v2, k + 1, lr_of_step(k + 1), beta1, beta2)
        for n, s in stats.items():
            var[n][2:] = moving_average(var[n][2:], s)
    return losses, var, g1
