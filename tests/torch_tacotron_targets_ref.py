"""float64 restatement of the reference's Tacotron graph WITH mel targets (tacotron/tacotron.py:36-37, :146-150): the decoder loop under
TacoTrainingHelper (tacotron/helpers.py:44-87) in both of its modes, for every attention type the port builds, and `add_loss`
(tacotron.py:258-282) in numpy float64.  Test infrastructure only: the checker of twv_tacotron_forward_targets / twv_tacotron_loss.

The graph around the helper is tests/torch_attention_ref.py's `infer` (its mechanism class and tests/torch_tacotron_ref.py's layer helpers are
imported, not copied); what differs is what TacoTrainingHelper decides:
  * the loop runs for T_out / r steps (helpers.py:55-59: the length of targets[:, r-1::r], the same for every utterance -- padding frames
    are not masked), not for max_iters;
  * step 0 is fed the zero go-frame (helpers.py:74-75, :90-92);
  * next_inputs (helpers.py:80-87): the last frame of the step's own output with rnn_decoder_test_mode, else targets[:, r-1::r][:, time].
Every layer is in inference mode in both modes (moving-average batch norm, no dropout), as in the library: the reference's training-mode
layers are outside this restatement.  Tolerance checker: float64, whatever order torch picks."""
import numpy as np
import torch

import torch_attention_ref as AR
import torch_tacotron_ref as R

F64 = R.F64


@torch.no_grad()
def forward_targets(w, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, t_out, teacher_forced):
    """returns (mel (N, t_out, M), linear (N, t_out, F), alignments (N, T_in, t_out / r)) float64 numpy.  mel_targets (N, t_out, M) or None
    when not teacher_forced."""
    tokens = np.asarray(tokens); lengths = np.asarray(lengths)
    RR, M = dims.r, dims.num_mels
    assert t_out % RR == 0 and t_out >= RR
    steps = t_out // RR
    fed = None
    if teacher_forced:
        tg = np.asarray(mel_targets, np.float64)
        assert tg.shape == (tokens.shape[0], t_out, M), tg.shape
        fed = torch.as_tensor(tg[:, RR - 1::RR, :])                # helpers.py:55: every r-th target frame
        assert fed.shape[1] == steps
    w = {k: R._t(v) for k, v in w.items()}
    N, T_in = tokens.shape
    multi = dims.n_speakers > 1
    table = R._t(w["embedding"]).clone()
    table[0] = 0.0
    x = table[torch.as_tensor(tokens, dtype=torch.long)]
    before_highway = enc_init = att_init = None
    dec_init = [None] * dims.dec_layers
    embed_to_concat = None
    if multi and getattr(dims, "model_simple", 0) and "speaker_embedding" in w and "dense_1/kernel" not in w:
        embed_to_concat = w["speaker_embedding"][torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)]
        linear_name = "dense"
    elif multi and "speaker_embedding" not in w:
        ids = torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)
        before_highway = w["before_highway"][ids]
        enc_init = w["encoder_rnn_init_state"][ids]
        att_init = w["attention_rnn_init_state"][ids]
        dec_init = [w["decoder_rnn_init_states%d" % (i + 1)][ids] for i in range(dims.dec_layers)]
        linear_name = "dense"
    elif multi:
        spk = R._t(w["speaker_embedding"])[torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)]
        softsign = lambda v: v / (v.abs() + 1.0)
        names = ["dense"] + ["dense_%d" % i for i in range(1, 3 + dims.dec_layers)]
        before_highway = R._dense(spk, w, names[0], softsign)
        enc_init = R._dense(spk, w, names[1], softsign)
        att_init = R._dense(spk, w, names[2], softsign)
        dec_init = [R._dense(spk, w, names[3 + i], softsign) for i in range(dims.dec_layers)]
        linear_name = "dense_%d" % (3 + dims.dec_layers)
    else:
        linear_name = "dense"
    h = R._dense(x, w, "prenet/dense_1", torch.relu)
    h = R._dense(h, w, "prenet/dense_2", torch.relu)
    enc = R._cbhg(h, lengths, w, "encoder_cbhg", dims.enc_bank, 2, dims.enc_hw_depth, before_highway, enc_init)
    mask = torch.as_tensor(np.arange(T_in)[None, :] < lengths[:, None])
    values = enc * mask[:, :, None].to(F64)
    keys = values @ R._t(w["memory_layer/kernel"])
    mech = AR._Mechanism(attention_type, w, keys, mask)
    AS = w["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
    att_h = att_init if att_init is not None else torch.zeros(N, AS, dtype=F64)
    dec_h = list(dec_init)
    context = torch.zeros(N, enc.shape[2], dtype=F64)
    state = mech.initial_state(N, T_in)
    frame = torch.zeros(N, M, dtype=F64)                           # helpers.py:75 _go_frames
    mel_steps, align_hist = [], []
    gp = "decoder/output_projection_wrapper/multi_rnn_cell/"
    for time in range(steps):
        p = R._dense(frame, w, "decoder/decoder_prenet/dense_1", torch.relu)
        p = R._dense(p, w, "decoder/decoder_prenet/dense_2", torch.relu)
        if embed_to_concat is not None:
            p = torch.cat([p, embed_to_concat], dim=-1)
        att_h = R._gru_cell(torch.cat([p, context], dim=-1), att_h, w, "decoder/attention_wrapper/gru_cell")
        align, state = mech(att_h, state)
        context = (align[:, None, :] @ values)[:, 0]
        align_hist.append(align)
        cat_out = [att_h, context] if embed_to_concat is None else [att_h, context, embed_to_concat]
        y = R._dense(torch.cat(cat_out, dim=-1), w, gp + "cell_0/output_projection_wrapper")
        for i in range(dims.dec_layers):
            if dec_h[i] is None:
                dec_h[i] = torch.zeros(N, y.shape[1], dtype=F64)
            dec_h[i] = R._gru_cell(y, dec_h[i], w, gp + "cell_%d/gru_cell" % (i + 1))
            y = y + dec_h[i]
        out = R._dense(y, w, "decoder/output_projection_wrapper")
        mel_steps.append(out.reshape(N, RR, M))
        # helpers.py:83-86 next_inputs
        frame = fed[:, time, :] if teacher_forced else out[:, -M:]
    mel = torch.cat(mel_steps, dim=1)
    post = R._cbhg(mel, None, w, "post_cbhg", dims.post_bank, 2, dims.post_hw_depth)
    linear = R._dense(post, w, linear_name)
    alignments = torch.stack(align_hist, dim=2)
    return mel.numpy(), linear.numpy(), alignments.numpy()


def add_loss(mel, linear, mel_targets, linear_targets, loss_coeff, prioritize_loss, sample_rate, num_freq):
    """tacotron.py:258-282 in numpy float64 from the float32 inputs: (loss, mel_loss, linear_loss, loss_without_coeff)"""
    mel, linear, mel_targets, linear_targets = [np.asarray(a, np.float32).astype(np.float64) for a in (mel, linear, mel_targets, linear_targets)]
    coeff = np.asarray(loss_coeff, np.float32).astype(np.float64)[:, None, None]       # expand_dims twice (:265)
    mel_l = np.abs(mel_targets - mel)
    l1 = np.abs(linear_targets - linear)
    if prioritize_loss:
        upper = int(5000 / (sample_rate * 0.5) * num_freq)
        lower = int(165 / (sample_rate * 0.5) * num_freq)
        pr = l1[:, :, lower:upper]
        loss = np.mean(mel_l * coeff) + 0.5 * np.mean(l1 * coeff) + 0.5 * np.mean(pr * coeff)
        linear_loss = 0.5 * (np.mean(l1) + np.mean(pr))
    else:
        loss = np.mean(mel_l * coeff) + np.mean(l1 * coeff)
        linear_loss = np.mean(l1)
    mel_loss = np.mean(mel_l)
    return float(loss), float(mel_loss), float(linear_loss), float(mel_loss + linear_loss)
